"""Memory safety of the native CPU code that decides results: the host entry points of the product (kh_host_* in csrc/common.hip,
csrc/join.hip, csrc/section.hip) and the oracle every bit-exact GPU comparison trusts (oracle/kimi_oracle.c), replayed under
AddressSanitizer and UBSan by the two stand-alone programs of tests/native_replay/ (helper: tests/native_replay.py).

The other host tests reach these functions through ctypes on numpy arrays, which live in the allocator's slack: a write one
element behind a buffer or a read at idx[n] gives the right answer there.  Here every array is a malloc of its own of exactly the
size the contract names (include/kimi_hip.h; for the oracle, what oracle/__init__.py allocates), outputs come pre-filled with a
canary, and every case asks three things:
  1. the sanitized program ends with status 0 and no sanitizer report;
  2. its return value and EVERY buffer are byte-identical to what the normal library (-O3 / -O2) gives through ctypes on the same
     bytes -- same source, -ffp-contract=off, no fast-math: a difference would mean the result depends on undefined behaviour;
  3. where the suite has a Python statement or a golden of the function, the result equals it, and entries the contract says are
     not written still hold the canary.
test_the_redzones_fire proves that a program built this way does fail on a write one element behind a buffer.

CPU only: nothing here is marked gpu, and the module skips itself where a GPU is present (sanitizer runs belong on the build
machine).  The sanitizers run in child processes; nothing sanitized is loaded into this interpreter."""
import ast
import collections
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: the sanitizer replays run on the CPU build machine only", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import native_replay as NR  # noqa: E402

if NR.hipcc() is None:
    pytest.skip("no hipcc", allow_module_level=True)
if NR.gcc() is None:
    pytest.skip("no gcc", allow_module_level=True)

import fill_ref  # noqa: E402
import join_ref as J  # noqa: E402
import section_ref  # noqa: E402
import shapes  # noqa: E402
from section_filled_ref import filled_mask  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
HOST, ORACLE = NR.HOST, NR.ORACLE
VOID = {"ko_weights26", "ko_set_voxel_graph", "ko_ball_radii", "ko_zero2inf", "ko_inf2zero"}     # the program reports 0 for these
CASES = collections.defaultdict(list)          # function -> the tests that replay it (test_every_symbol_has_a_case)
REPLAYED = collections.Counter()               # function -> replays so far in this process
u8, u16, u32, u64, i32, i64, f32, f64 = (np.uint8, np.uint16, np.uint32, np.uint64, np.int32, np.int64, np.float32, np.float64)
ANISOTROPIES = ((1, 1, 1), (16, 16, 40))
SHAPE = (24, 20, 16)


def replays(*functions):
    """names the functions a test replays; the test fails if it ends without having replayed each of them"""
    def mark(test):
        for f in functions:
            CASES[f].append(test.__name__)

        @functools.wraps(test)
        def run(*args, **kwargs):
            before = {f: REPLAYED[f] for f in functions}
            test(*args, **kwargs)
            assert all(REPLAYED[f] > before[f] for f in functions), "a function named in @replays was not replayed"
        return run
    return mark


@functools.lru_cache(maxsize=None)
def library(program):
    if program == ORACLE:
        import oracle
        return oracle.lib()
    from kimimaro_amd import _abi, build
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def both_many(program, calls):
    """calls = [(function, arguments in the C parameter order: int / float scalars, numpy arrays, None = NULL), ...], made in order on
    ONE set of buffers (an array object named twice is one buffer) by the sanitized program and, on copies, by the normal library.
    Asserts points 1 and 2 of the module docstring.  -> ([return values], after) with after(array) = that buffer after the calls."""
    lib = library(program)
    arrays, index, file_calls = [], {}, []
    for function, args in calls:
        scalars, where = [], []
        for a in args:
            if a is None:
                where.append(None)
            elif isinstance(a, np.ndarray):
                if id(a) not in index:
                    index[id(a)] = len(arrays)
                    arrays.append(a)
                where.append(index[id(a)])
            else:
                assert isinstance(a, (int, float, np.integer, np.floating)), a
                scalars.append(a)
        file_calls.append((function, scalars, where))
    sanitized_rets, sanitized = NR.run(program, arrays, file_calls)
    mine = [a.copy(order="K") for a in arrays]
    normal_rets = []
    for function, args in calls:
        fn = getattr(lib, function)
        cargs = []
        for a in args:
            if a is None:
                cargs.append(None)
            elif isinstance(a, np.ndarray):
                cargs.append(C.c_void_p(mine[index[id(a)]].ctypes.data))
            else:
                cargs.append(int(a) if isinstance(a, (int, np.integer)) else float(a))
        r = fn(*cargs)
        normal_rets.append(0 if function in VOID else int(r))
        REPLAYED[function] += 1
    names = [c[0] for c in calls]
    assert sanitized_rets == normal_rets, (names, sanitized_rets, normal_rets)
    for k, (s, n) in enumerate(zip(sanitized, mine)):
        assert s.tobytes(order="A") == n.tobytes(order="A"), "%s: buffer %d differs between the sanitized -O1 build and the library" % (names, k)
    return normal_rets, lambda a: mine[index[id(a)]]


def both(program, function, args):
    rets, after = both_many(program, [(function, args)])
    return rets[0], after


def fortran(a, dtype=None):
    return np.asfortranarray(a, dtype=dtype)


# ---- the harness itself -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("program", [HOST, ORACLE])
def test_the_redzones_fire(program):
    """a write one element behind an exact-size output buffer, and one into a zero-length buffer, end the program with a
    heap-buffer-overflow report: the redzones are active, so a clean case means something"""
    for count, dtype in ((5, u32), (0, u64)):
        status, err = NR.run(program, [NR.canary(count, dtype)], [("selftest_overrun", [], [0])], expect_failure=True)
        assert status != 0 and "heap-buffer-overflow" in err, (count, status, err)
    with pytest.raises(NR.ReplayFailure, match="heap-buffer-overflow"):
        NR.call(program, "selftest_overrun", [], [NR.canary(3, f32)])


def test_call_returns_the_whole_buffers():
    lab = fortran(np.arange(6).reshape(3, 2, 1) % 2, u8)
    ret, (lab_after, out) = NR.call(HOST, "kh_host_ccl26", [1, 3, 2, 1], [lab, NR.canary(6, u32, (3, 2, 1))])
    assert ret == 1 and np.array_equal(lab_after, lab) and out.shape == (3, 2, 1) and out.flags.f_contiguous
    assert out.ravel(order="F").tolist() == [0, 0, 0, 1, 1, 1]
    ret, (none, out) = NR.call(HOST, "kh_host_ccl26", [3, 3, 2, 1], [None, NR.canary(6, u32)])     # refused before anything is read
    assert ret == -1 and none is None and NR.is_canary(out)


# ---- kh_host_ccl26 / ko_ccl26 -----------------------------------------------------------------------------------------------------

CCL_SHAPES = ((1, 1, 1), (7, 1, 1), (1, 9, 1), (5, 4, 3))


def ccl_volumes(dtype):
    rng = np.random.default_rng(3)
    for shape in CCL_SHAPES:
        top = int(np.iinfo(dtype).max)
        values = np.array([0, 1, top], dtype=dtype)
        yield fortran(values[rng.integers(0, 3, shape)])
        yield np.zeros(shape, dtype=dtype, order="F")
        yield np.full(shape, top, dtype=dtype, order="F")


def components_by_scipy(lab):
    """26-connected components of equal non-zero value, ids 1..N by first appearance in the F-order raster"""
    import scipy.ndimage as ndi
    out = np.zeros(lab.shape, dtype=np.int64)
    n = 0
    for v in np.unique(lab[lab != 0]).tolist():
        comp, k = ndi.label(lab == v, structure=np.ones((3, 3, 3)))
        out[comp > 0] = comp[comp > 0] + n
        n += k
    flat = out.ravel(order="F")
    ids, first = np.unique(flat[flat > 0], return_index=True)
    rank = np.zeros(n + 1, dtype=np.int64)
    rank[ids[np.argsort(first)]] = np.arange(1, ids.size + 1)
    return rank[out].astype(u32), n


@replays("kh_host_ccl26")
@pytest.mark.parametrize("dtype", [u8, u16, u32, u64])
def test_host_ccl26(dtype):
    for lab in ccl_volumes(dtype):
        out = NR.canary(lab.size, u32, lab.shape)
        n, after = both(HOST, "kh_host_ccl26", [lab, lab.itemsize, *lab.shape, out])
        want, want_n = components_by_scipy(lab)
        assert n == want_n and np.array_equal(after(out), want), lab.shape


@replays("kh_host_ccl26")
def test_host_ccl26_refuses_three_byte_labels():
    lab, out = np.ones(3 * 60, dtype=u8), NR.canary(60, u32)
    n, after = both(HOST, "kh_host_ccl26", [lab, 3, 5, 4, 3, out])
    assert n == -1 and NR.is_canary(after(out))


@replays("ko_ccl26")
@pytest.mark.parametrize("dtype", [u8, u16, u32, u64])
def test_oracle_ccl26(dtype):
    for lab in ccl_volumes(dtype):
        out = NR.canary(lab.size, u32, lab.shape)
        n, after = both(ORACLE, "ko_ccl26", [lab, lab.itemsize, *lab.shape, out])
        want, want_n = components_by_scipy(lab)
        assert n == want_n and np.array_equal(after(out), want), lab.shape


# ---- kh_host_consolidate_paths ----------------------------------------------------------------------------------------------------

def consolidate(res, shape):
    """the call with outputs of exactly sum(lens) vertices / edges -> (return value, {name: whole output buffer})"""
    voff, loff = np.asarray(res["voff"], dtype=i64), np.asarray(res["loff"], dtype=i64)
    locs, lens, radii = np.asarray(res["verts"], dtype=u32), np.asarray(res["lens"], dtype=u32), np.asarray(res["radii"], dtype=f32)
    n, nslots = int(lens.sum()), voff.size - 1
    assert n == locs.size == radii.size
    out = {"verts": NR.canary(3 * n, f32).reshape(n, 3), "radii": NR.canary(n, f32), "edges": NR.canary(2 * n, u32).reshape(n, 2),
           "vstart": NR.canary(nslots + 1, i64), "estart": NR.canary(nslots + 1, i64)}
    got, after = both(HOST, "kh_host_consolidate_paths", [nslots, voff, loff, locs, lens, radii, *shape, out["verts"], out["radii"],
                                                          out["edges"], out["vstart"], out["estart"]])
    return got, {k: after(v) for k, v in out.items()}


def assert_consolidated(res, shape):
    from kimimaro_amd import intake
    got, out = consolidate(res, shape)
    want = intake.consolidate_paths_flat_numpy({k: np.asarray(v) for k, v in res.items()}, shape)
    nv, ne = int(out["vstart"][-1]), int(out["estart"][-1])
    assert got == nv == len(want["verts"]) and ne == len(want["edges"])
    for k, n in (("verts", nv), ("radii", nv), ("edges", ne)):
        assert np.array_equal(out[k][:n], np.asarray(want[k])), k
        assert NR.is_canary(out[k][n:]), k                                    # nothing behind the rows the call reports
    assert np.array_equal(out["vstart"], want["vstart"]) and np.array_equal(out["estart"], want["estart"])
    return out


@replays("kh_host_consolidate_paths")
def test_host_consolidate_paths_edges():
    shape = (7, 5, 3)
    a, b, c, d, e, g, h = 3, 17, 40, 41, 77, 90, 104
    slots = [[[a, b]],                                        # an ordinary slot in front (the statement's path ends are cumulative)
             [],                                              # a slot without paths
             [[], [c], [a, a, b, c], [c, d, a], [e]],         # lengths 0 and 1, a voxel repeated consecutively, two paths sharing vertices
             [[g], [h, h], [g]],                              # every vertex is dropped: one-vertex paths and a self loop
             [[h, g, e, d]]]
    voff, loff, locs, lens = [0], [0], [], []
    for paths in slots:
        for p in paths:
            locs += p
            lens.append(len(p))
        voff.append(len(locs))
        loff.append(len(lens))
    radii = np.arange(1, len(locs) + 1, dtype=f32)            # all different: the radius names the occurrence it came from
    out = assert_consolidated({"voff": voff, "loff": loff, "verts": locs, "lens": lens, "radii": radii}, shape)
    assert np.diff(out["vstart"]).tolist() == [2, 0, 4, 0, 4] and np.diff(out["estart"]).tolist() == [1, 0, 4, 0, 3]
    # slot 2, sorted by (x, y, z): a = (3,0,0), b = (3,2,0), c = (5,0,1), d = (6,0,1); e has no edge.  First occurrences: c in the
    # one-vertex path (radius 3), a and b in the third path (radii 4 and 6), d in the fourth (radius 9)
    assert out["verts"][2:6].tolist() == [[3, 0, 0], [3, 2, 0], [5, 0, 1], [6, 0, 1]]
    assert out["radii"][2:6].tolist() == [4, 6, 3, 9]
    assert out["edges"][1:5].tolist() == [[0, 1], [0, 3], [1, 2], [2, 3]]


@replays("kh_host_consolidate_paths")
def test_host_consolidate_paths_without_slots_and_without_vertices():
    empty = {"voff": [0], "loff": [0], "verts": [], "lens": [], "radii": []}
    got, out = consolidate(empty, (4, 4, 4))
    assert got == 0 and out["vstart"].tolist() == [0] and out["estart"].tolist() == [0]
    got, out = consolidate({"voff": [0, 0, 0], "loff": [0, 0, 2], "verts": [], "lens": [0, 0], "radii": []}, (4, 4, 4))
    assert got == 0 and out["vstart"].tolist() == [0, 0, 0] and out["estart"].tolist() == [0, 0, 0]


@replays("kh_host_consolidate_paths")
@pytest.mark.parametrize("seed,shape", [(1, (7, 5, 3)), (0, (40, 37, 29))])
def test_host_consolidate_paths_random(seed, shape):
    """the generator of tests/test_host.py: repeated vertices, self loops, one-vertex paths and empty slots"""
    rng = np.random.default_rng(seed)
    nvox = int(np.prod(shape))
    voff, loff, locs, lens = [0], [0], [], []
    for s in range(60):
        for p in range(int(rng.integers(0, 5))):
            n = int(rng.integers(1, 30))
            pts = rng.integers(0, max(nvox // 50, 2), n) * rng.integers(1, 3)
            locs.extend(int(v) % nvox for v in pts)
            lens.append(n)
        voff.append(len(locs))
        loff.append(len(lens))
    assert_consolidated({"voff": voff, "loff": loff, "verts": locs, "lens": lens, "radii": rng.random(len(locs)).astype(f32)}, shape)


# ---- kh_host_merge_components -----------------------------------------------------------------------------------------------------

MERGE_SHAPE = (9, 8, 7)


def merge_statement(pol, vstart, estart, V, R, E, an):
    """Skeleton.simple_merge(parts).consolidate() per label on disjoint, already consolidated parts: the vertices re-sorted by
    (x, y, z) and scaled, the edges renumbered and sorted as rows (lo, hi)"""
    oV, oR, oE = np.zeros_like(V), np.zeros_like(R), np.zeros_like(E)
    for l in range(len(pol) - 1):
        p0, p1 = int(pol[l]), int(pol[l + 1])
        if p1 <= p0:
            continue
        v0, v1, e0, e1 = int(vstart[p0]), int(vstart[p1]), int(estart[p0]), int(estart[p1])
        verts = V[v0:v1]
        order = np.lexsort((verts[:, 2], verts[:, 1], verts[:, 0]))
        rank = np.empty(v1 - v0, dtype=np.int64)
        rank[order] = np.arange(v1 - v0)
        oV[v0:v1] = np.multiply(verts[order], an, dtype=f32)
        oR[v0:v1] = R[v0:v1][order]
        rows = [rank[E[int(estart[p]):int(estart[p + 1])].astype(np.int64) + (int(vstart[p]) - v0)] for p in range(p0, p1)]
        rows = np.concatenate(rows).reshape(-1, 2)
        rows = np.stack([rows.min(axis=1), rows.max(axis=1)], axis=1) if rows.size else rows
        oE[e0:e1] = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    return oV, oR, oE


@replays("kh_host_merge_components")
def test_host_merge_components():
    rng = np.random.default_rng(17)
    sx, sy, sz = MERGE_SHAPE
    pool, taken = rng.permutation(sx * sy * sz), [0]

    def part(nv, edges="tree", shuffle=False):
        key = np.sort(pool[taken[0]:taken[0] + nv])
        taken[0] += nv
        if shuffle:
            key = key[::-1].copy()
        verts = np.stack([key // (sy * sz), (key // sz) % sy, key % sz], axis=1).astype(f32)
        if edges == "tree" and nv > 1:
            e = np.stack([[int(rng.integers(0, i)) for i in range(1, nv)], np.arange(1, nv)], axis=1)
        elif edges == "star" and nv > 1:
            e = np.stack([np.zeros(nv - 1, dtype=np.int64), np.arange(1, nv)], axis=1)     # every edge shares its lo
        else:
            e = np.zeros((0, 2), dtype=np.int64)
        e = e[np.lexsort((e[:, 1], e[:, 0]))].astype(u32)
        return verts.reshape(-1, 3), e, rng.random(nv).astype(f32)

    labels = [[],                                                         # a label with no parts
              [part(9)],                                                  # one part: the copy branch
              [part(7), part(5), part(11)],                               # three sorted parts: the merge branch
              [part(6), part(8, shuffle=True), part(4)],                  # one part unsorted: the full-sort branch
              [part(0, edges=None), part(5, edges=None), part(3)],        # a part without vertices, a part without edges
              [part(9, edges="star"), part(7, edges="star")],             # several edges per lo: the insertion sort
              []]
    parts = [p for parts_of_label in labels for p in parts_of_label]
    pol = np.concatenate([[0], np.cumsum([len(l) for l in labels])]).astype(i64)
    vstart = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(i64)
    estart = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).astype(i64)
    V, E, R = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(3))
    for an in ((1, 1, 1), (16, 16, 40), (0.5, 1.25, 3)):
        an = np.array(an, dtype=f32)
        oV, oR, oE = NR.canary(V.size, f32).reshape(V.shape), NR.canary(R.size, f32), NR.canary(E.size, u32).reshape(E.shape)
        got, after = both(HOST, "kh_host_merge_components", [len(labels), pol, vstart, estart, V, R, E, sy, sz, float(an[0]), float(an[1]),
                                                             float(an[2]), oV, oR, oE])
        wV, wR, wE = merge_statement(pol, vstart, estart, V, R, E, an)
        assert got == 0
        assert np.array_equal(after(oV), wV) and np.array_equal(after(oR), wR) and np.array_equal(after(oE), wE)
    # nothing at all: every array has zero length but part_of_label
    zero = lambda dtype, *shape: np.zeros(shape or (0,), dtype=dtype)
    got, _ = both(HOST, "kh_host_merge_components", [0, zero(i64, 1), zero(i64, 1), zero(i64, 1), zero(f32, 0, 3), zero(f32), zero(u32, 0, 2), sy,
                                                     sz, 1.0, 1.0, 1.0, NR.canary(0, f32), NR.canary(0, f32), NR.canary(0, u32)])
    assert got == 0


# ---- kh_host_find_border_targets --------------------------------------------------------------------------------------------------

def border_targets(dt, cc, wx, wy, nlab, order_entries=None):
    """the call with the caller's sizes (kimimaro_amd/border.py): out_xy 2 * (nlab + 1) floats, order nlab + 1 entries ->
    ({id: (x, y)} in the order reported, the out_xy rows as left by the call)"""
    dt, cc = fortran(dt, f32), fortran(cc, u32)
    xy = NR.canary(2 * (nlab + 1), f32)
    order = NR.canary(nlab + 1 if order_entries is None else order_entries, i32)
    n, after = both(HOST, "kh_host_find_border_targets", [dt, cc, dt.shape[0], dt.shape[1], float(wx), float(wy), nlab, xy, order])
    xy, order = after(xy).reshape(-1, 2), after(order)
    assert 0 <= n <= nlab and NR.is_canary(order[n:])
    ids = order[:n].tolist()
    unwritten = np.array([l for l in range(nlab + 1) if l not in ids], dtype=np.int64)
    assert NR.is_canary(xy[unwritten])                                          # the rows of ids without a maximum are not written
    return {l: (int(xy[l, 0]), int(xy[l, 1])) for l in ids}


def assert_border_statement(dt, cc, wx, wy, nlab, **kw):
    from oracle.border import find_border_targets
    got = border_targets(dt, cc, wx, wy, nlab, **kw)
    want = find_border_targets(fortran(dt, f32), fortran(cc, u32), wx, wy)
    assert list(got) == [int(k) for k in want]
    for k, v in want.items():
        assert got[int(k)] == (int(v[0]), int(v[1])), k
    return got


@replays("kh_host_find_border_targets")
def test_host_find_border_targets_golden():
    z = np.load(os.path.join(G, "border_targets.npz"))
    for i in range(int(z["n"])):
        cc, dt = z["cc_%d" % i], z["dt_%d" % i]
        wx, wy = z["w_%d" % i]
        got = border_targets(dt, cc, wx, wy, int(cc.max()))
        assert list(got) == z["keys_%d" % i].tolist(), i
        assert [got[k] for k in got] == [tuple(v) for v in z["vals_%d" % i].tolist()], i


@replays("kh_host_find_border_targets")
@pytest.mark.parametrize("pitch", [(1, 1), (16, 40), (0.5, 3)])
def test_host_find_border_targets_edges(pitch):
    wx, wy = pitch
    rng = np.random.default_rng(23)
    # no component at all: nothing is written, an `order` of no entries is enough
    assert assert_border_statement(np.ones((4, 3)), np.zeros((4, 3)), wx, wy, 0, order_entries=0) == {}
    # component 2 has no non-zero distance anywhere: it is not reported and its row stays untouched; id 3 does not occur
    cc = np.zeros((9, 7), dtype=u32)
    cc[0:4, 0:3], cc[5:9, 2:7] = 1, 2
    dt = np.where(cc == 1, rng.integers(1, 4, cc.shape), 0)
    assert list(assert_border_statement(dt, cc, wx, wy, 3)) == [1]
    # planes that are one row or one column
    for shape in ((11, 1), (1, 11)):
        cc = np.ones(shape, dtype=u32)
        cc.reshape(-1)[4:6] = 0
        cc.reshape(-1)[6:] = 2
        for dt in (np.ones(shape), rng.integers(0, 3, shape)):
            assert_border_statement(dt, cc, wx, wy, 2)
    # exact ties: one plateau, the tie-break decides everything (blocks as in tests/test_oracle_vs_ref.py)
    for t in range(6):
        sx, sy = int(rng.integers(3, 14)), int(rng.integers(3, 14))
        cc = np.zeros((sx, sy), dtype=u32)
        for l in range(1, 5):
            x0, y0 = int(rng.integers(0, sx)), int(rng.integers(0, sy))
            cc[x0:int(rng.integers(x0, sx)) + 1, y0:int(rng.integers(y0, sy)) + 1] = l
        dt = np.ones((sx, sy)) if t % 2 else np.floor(rng.random((sx, sy)) * 3)
        assert_border_statement(dt, cc, wx, wy, 4)


# ---- kh_host_resolve_holes / kh_host_enclosed_regions -----------------------------------------------------------------------------

def hole_volumes():
    from test_gpu_fill_holes import _box_wall, _nested
    yield "nested, outer first", _nested(1, 2)
    yield "nested, inner first", _nested(2, 1)
    for shell_id, thread_id in ((1, 2), (2, 1)):
        cc = np.zeros((16, 16, 12), dtype=u32)
        _box_wall(cc, (2, 2, 2), (8, 8, 8), shell_id)
        for k in range(5, 11):
            cc[k, k, 5] = thread_id
        cc[10:13, 10:13, 4:7] = thread_id
        cc[11, 11, 5] = 0
        yield "diagonal thread %d through shell %d" % (thread_id, shell_id), cc
    cc = np.zeros((12, 12, 12), dtype=u32)
    _box_wall(cc, (0, 3, 3), (6, 9, 9), 4)
    cc[0, 4:9, 4:9] = 0
    yield "box open at the face", cc
    cc = np.zeros((14, 14, 14), dtype=u32)
    cc[fill_ref.shell(cc.shape, (1.0, 7.0, 7.0), 5.0, 1.5)] = 6
    yield "sphere cut by the face", cc
    cc = np.zeros((14, 14, 14), dtype=u32)
    _box_wall(cc, (0, 3, 3), (6, 9, 9), 4)
    yield "box closed on the face", cc
    wide = _nested(1, 2).astype(u64) * u64((1 << 33) + 5)               # label words above 2^32
    yield "values above 2^32", wide
    for seed in (0, 1, 2, 3, 5, 8):
        yield "random %d" % seed, fill_ref.random_volume(seed)


def resolve(value, count, face, pairs, nregions=None, null_pairs=False):
    """the call with the header's sizes -> (return value, owner, label_value, label_state, filled) as left by the call"""
    nreg = value.size - 1 if nregions is None else nregions
    owner, label_value, label_state, filled = NR.canary(nreg + 1, u64), NR.canary(nreg, u64), NR.canary(nreg, u8), NR.canary(1, i64)
    n, after = both(HOST, "kh_host_resolve_holes", [nreg, value, count, face, pairs.size, None if null_pairs else pairs, owner,
                                                    label_value, label_state, filled])
    return n, after(owner), after(label_value), after(label_state), after(filled)


def enclosed(value, face, pairs, wanted, capacity, nregions=None, null_pairs=False, null_regions=False):
    nreg = value.size - 1 if nregions is None else nregions
    wanted = np.asarray(wanted, dtype=u64)
    offsets, regions = NR.canary(wanted.size + 1, u64), NR.canary(capacity, u32)
    n, after = both(HOST, "kh_host_enclosed_regions", [nreg, value, face, pairs.size, None if null_pairs else pairs, wanted.size, wanted,
                                                       offsets, None if null_regions else regions, capacity])
    return n, after(offsets), None if null_regions else after(regions)


@replays("kh_host_resolve_holes", "kh_host_enclosed_regions")
def test_host_region_graphs_of_the_fill_holes_volumes():
    for name, cc in hole_volumes():
        value, count, face, pairs, region = fill_ref.region_graph(cc)
        want_volume, want_filled, want_state = fill_ref.static(cc)
        n, owner, label_value, label_state, filled = resolve(value, count, face, pairs)
        labels = np.unique(cc[cc != 0])
        assert n == labels.size and np.array_equal(label_value[:n], labels.astype(u64)), name
        assert NR.is_canary(label_value[n:]) and NR.is_canary(label_state[n:]), name         # only the first `return value` entries are set
        assert {int(k): int(s) for k, s in zip(label_value[:n], label_state[:n])} == want_state, name
        assert int(filled[0]) == want_filled and np.array_equal(fill_ref.owner_volume(cc, owner, region), want_volume), name
        # hole(L) for every label, an absent one, a duplicate and 0; first the size, then exact, then one too small
        wanted = labels.tolist() + [int(labels.max()) + 7, int(labels[-1]), 0]
        total, offsets, _ = enclosed(value, face, pairs, wanted, 0, null_regions=True)
        assert offsets[0] == 0 and offsets[-1] == total and np.all(np.diff(offsets.astype(i64)) >= 0), name
        again, offsets2, regions = enclosed(value, face, pairs, wanted, total)
        assert again == total and np.array_equal(offsets, offsets2), name
        for k, L in enumerate(wanted):
            mine = regions[int(offsets[k]):int(offsets[k + 1])]
            assert np.all(mine[1:] > mine[:-1]), (name, L)
            assert np.array_equal(np.isin(region, mine), filled_mask(cc, L) & (cc != L)), (name, L)
        assert offsets[len(labels) + 1] == offsets[len(labels)]                                # the absent label: an empty range
        if total > 0:
            short, offsets3, untouched = enclosed(value, face, pairs, wanted, total - 1)
            assert short == total and np.array_equal(offsets, offsets3) and NR.is_canary(untouched), name


@replays("kh_host_resolve_holes", "kh_host_enclosed_regions")
def test_host_region_graph_edges():
    value, count, face = np.array([0, 0, 1], dtype=u64), np.array([0, 20, 7], dtype=u32), np.array([0, 1, 0], dtype=u8)
    none = np.zeros(0, dtype=u64)
    # no regions: the tables have their entry 0 only
    n, owner, _, _, filled = resolve(value[:1], count[:1], face[:1], none, null_pairs=True)
    assert n == 0 and owner.tolist() == [0] and filled.tolist() == [0]
    total, offsets, _ = enclosed(value[:1], face[:1], none, [3, 0], 0, null_pairs=True, null_regions=True)
    assert total == 0 and offsets.tolist() == [0, 0, 0]
    total, offsets, _ = enclosed(value[:1], face[:1], none, [], 0, null_pairs=True, null_regions=True)
    assert total == 0 and offsets.tolist() == [0]
    # regions without pairs, pairs == NULL: region 2 touches no face and no neighbour, nothing encloses it
    n, owner, label_value, label_state, filled = resolve(value, count, face, none, null_pairs=True)
    assert n == 1 and owner.tolist() == [0, 0, 0] and label_value[:n].tolist() == [1] and label_state[:n].tolist() == [fill_ref.PROCESSED]
    assert filled.tolist() == [0] and NR.is_canary(label_value[n:]) and NR.is_canary(label_state[n:])
    total, offsets, _ = enclosed(value, face, none, [1, 1, 0], 0, null_pairs=True, null_regions=True)
    assert total == 0 and offsets.tolist() == [0, 0, 0, 0]
    # pairs that name region 0, a region above nregions, or one region twice: -2, nothing is written
    good = np.array([(1 << 32) | 2], dtype=u64)
    for bad in (2, (1 << 32) | 3, (3 << 32) | 1, (2 << 32) | 2, 0):
        pairs = np.array([good[0], bad], dtype=u64)
        n, owner, label_value, label_state, filled = resolve(value, count, face, pairs)
        assert n == -2 and all(NR.is_canary(a) for a in (owner, label_value, label_state, filled)), bad
        total, offsets, regions = enclosed(value, face, pairs, [1], 4)
        assert total == -2 and NR.is_canary(offsets) and NR.is_canary(regions), bad
    # the one good pair: region 2 (label 1) hangs on face-owning background, no holes
    n, owner, _, label_state, _ = resolve(value, count, face, good)
    assert n == 1 and owner.tolist() == [0, 0, 0] and label_state[:n].tolist() == [fill_ref.PROCESSED]


# ---- kh_host_join_plan ------------------------------------------------------------------------------------------------------------

def plan(sizes, d2, idx, radii, radius, restrict, edge_entries=None):
    sizes = np.ascontiguousarray(sizes, dtype=u32)
    d2 = np.ascontiguousarray(d2, dtype=f64).view(u64)
    idx, radii = np.ascontiguousarray(idx, dtype=u32), np.ascontiguousarray(radii, dtype=f32)
    n = sizes.size
    edges = NR.canary(2 * max(n - 1, 0) if edge_entries is None else edge_entries, u32)
    m, after = both(HOST, "kh_host_join_plan", [n, sizes, d2, idx, radii, float(radius), int(restrict), edges])
    return m, after(edges).reshape(-1, 2)


def assert_plan(skeletons, radius, restrict):
    parts = J.parts_of(skeletons)
    sizes, d2, idx, _, radii, r = J.tables_of(parts, radius, restrict)
    want = J.plan(sizes, d2, idx, radii, r, restrict)
    m, edges = plan(sizes, d2, idx, radii, r, restrict)
    assert m == len(want) and np.array_equal(edges[:m], want) and NR.is_canary(edges[m:])
    return want


@replays("kh_host_join_plan")
def test_host_join_plan_edges():
    from test_join_host import LATTICES, MODES, line
    # no part, one part: 0, and no array is looked at -- each has zero length
    zero = lambda dtype: np.zeros(0, dtype=dtype)
    for n in (0, 1):
        edges = NR.canary(0, u32)
        m, _ = both(HOST, "kh_host_join_plan", [n, zero(u32), zero(u64), zero(u32), zero(f32), float("inf"), 0, edges])
        assert m == 0
    assert assert_plan([line(0, 3), line(5, 2)], np.inf, False).tolist() == [[2, 3]]                    # two parts
    assert len(assert_plan([line(0, 3), line(10, 3), line(20, 3)], 2.0, False)) == 0                    # every record none
    thin = [line(0, 3, r=0.5), line(4, 3, r=0.5)]
    thin[0].radii[0] = 3.0
    assert len(assert_plan(thin, np.inf, True)) == 0                                                    # restrict_by_radius rejects
    assert assert_plan([line(0, 3, r=1.5), line(4, 3, r=1.5)], np.inf, True).tolist() == [[2, 3]]       # ... and accepts
    # a record that is not none names a vertex outside its part: -1, nothing is written
    sizes, d2 = [3, 2], np.array([[np.inf, 4.0], [4.0, np.inf]])
    idx = np.array([[[J.NONE, J.NONE], [2, 0]], [[0, 2], [J.NONE, J.NONE]]], dtype=u32)
    m, edges = plan(sizes, d2, idx, np.ones(5, dtype=f32), np.inf, 0)
    assert m == 1 and edges.tolist() == [[2, 3]]
    for cell, col in (((0, 1), 0), ((0, 1), 1), ((1, 0), 0), ((1, 0), 1)):
        bad = idx.copy()
        bad[cell][col] = 3 if (cell == (0, 1)) == (col == 0) else 2
        m, edges = plan(sizes, d2, bad, np.ones(5, dtype=f32), np.inf, 0)
        assert m == -1 and NR.is_canary(edges), (cell, col)
    # exact key ties: fragments on integer lattices
    merged = 0
    for lattice in LATTICES:
        frags = J.fragments(1, **lattice)
        for radius, restrict in MODES + ((3.0 * max(lattice.get("anisotropy", (1,))), False),):
            merged += len(assert_plan(frags, radius, restrict))
    assert merged > 0


@replays("kh_host_join_plan")
def test_host_join_plan_golden():
    """the join cases of tests/golden/post.npz, as tests/test_join_host.py feeds them"""
    from kimimaro_amd import post
    from test_join_host import golden_input, golden_vectors
    from test_post import GOLD
    for i in golden_vectors("join_close_components"):
        args = ast.literal_eval(str(GOLD["args_%d" % i]))
        assert_plan(golden_input(i), np.inf if args[0] is None else args[0], args[1])
    for i in golden_vectors("postprocess"):
        args = ast.literal_eval(str(GOLD["args_%d" % i]))
        skel = post.remove_loops(post.remove_dust(golden_input(i).consolidate(remove_disconnected_vertices=True), args[0]))
        assert_plan(skel, np.inf, True)


# ---- kh_host_section_voxel --------------------------------------------------------------------------------------------------------

@replays("kh_host_section_voxel")
@pytest.mark.parametrize("anisotropy", [(1, 1, 1), (4, 4, 40), (0.5, 1.25, 3)])
def test_host_section_voxel(anisotropy):
    from test_gpu_section import LATTICE, NEAR
    rng = np.random.default_rng(29)
    an = np.array(anisotropy, dtype=f64)
    normals = [np.array(v, dtype=f64) for v in LATTICE + NEAR]
    normals = [v / np.sqrt(v @ v) for v in normals] + [np.array([3.0, 0, 0])]            # ... and one that is not a unit vector
    corners = [(-3, -3, -3), (3, 3, 3), (0, 0, 0)]                   # the ends of the offsets' range, the seed itself
    for n in normals:
        deltas = np.array(corners + rng.integers(-3, 4, size=(1, 3)).tolist())
        want_d, want_h = section_ref.offsets(n, an, deltas), section_ref.half_width(n, an)
        want_area = section_ref.voxel_areas(n, an, want_d)
        for k, delta in enumerate(deltas.tolist()):
            d, h, area = NR.canary(1, f64), NR.canary(1, f64), NR.canary(1, f64)
            cut, after = both(HOST, "kh_host_section_voxel", [n, an, *delta, d, h, area])
            assert after(d)[0] == want_d[k] and after(h)[0] == want_h and cut == int(abs(want_d[k]) < want_h)
            if cut:
                assert abs(after(area)[0] - want_area[k]) <= 1e-12 * max(anisotropy) ** 2      # the bound of tests/test_section_host.py


# ---- the oracle: small helpers ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tube():
    m = shapes.random_walk_tube(SHAPE, 7)
    m.setflags(write=False)
    return m


def tube_centre():
    """(x, y, z) of a voxel in the middle of the tube's voxel list: the slices through it are not empty"""
    inside = np.flatnonzero(tube().ravel(order="F"))
    loc = int(inside[inside.size // 2])
    return loc % SHAPE[0], (loc // SHAPE[0]) % SHAPE[1], loc // (SHAPE[0] * SHAPE[1])


def unpack(bits, shape):
    n = int(np.prod(shape))
    return fortran(np.unpackbits(bits)[:n].reshape(shape, order="F").astype(u8))


def lin(pts, shape):
    pts = np.asarray(pts, dtype=i64).reshape(-1, 3)
    return (pts[:, 0] + shape[0] * (pts[:, 1] + shape[1] * pts[:, 2])).astype(u64)


def random_graph(shape, seed, keep=0.9):
    rng = np.random.default_rng(seed)
    g = np.zeros(shape, dtype=u32, order="F")
    for bit in range(26):
        g |= (rng.random(shape) < keep).astype(u32) << u32(bit)
    return g


@replays("ko_weights26")
def test_oracle_weights26():
    import oracle
    for an in ANISOTROPIES + ((0.5, 1.25, 3),):
        w = NR.canary(26, f32)
        _, after = both(ORACLE, "ko_weights26", [float(an[0]), float(an[1]), float(an[2]), w])
        d = np.abs(np.array(oracle._DIRS, dtype=f32)) * np.array(an, dtype=f32)
        sq = d * d
        assert np.array_equal(after(w), np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2], dtype=f32))


@replays("ko_zero2inf", "ko_inf2zero", "ko_first_label")
def test_oracle_small_helpers():
    rng = np.random.default_rng(31)
    f = rng.integers(0, 3, 211).astype(f32)
    f[rng.random(211) < 0.2] = np.inf
    f[5], f[6] = -0.0, -np.inf
    for a in (f, np.zeros(0, dtype=f32), np.zeros(1, dtype=f32)):
        _, after = both(ORACLE, "ko_zero2inf", [a, a.size])
        assert np.array_equal(after(a), np.where(a == 0, f32(np.inf), a))
        _, after = both(ORACLE, "ko_inf2zero", [a, a.size])
        assert np.array_equal(after(a), np.where(a == np.inf, f32(0), a))
    z = np.load(os.path.join(G, "legacy_targets.npz"))
    for i in range(int(z["n"])):
        shape = tuple(int(v) for v in z["shape_%d" % i])
        mask = unpack(z["mask_%d" % i], shape)
        first, _ = both(ORACLE, "ko_first_label", [mask, mask.size])
        want = tuple(int(v) for v in z["first_%d" % i])
        assert first == (-1 if want == (-1, -1, -1) else int(lin(want, shape)[0])), i
    for mask in (np.zeros(0, dtype=u8), np.zeros(7, dtype=u8), np.array([0, 0, 3], dtype=u8)):
        first, _ = both(ORACLE, "ko_first_label", [mask, mask.size])
        assert first == (2 if mask.any() else -1)


# ---- the oracle: EDT --------------------------------------------------------------------------------------------------------------

def edt_by_scipy(lab, an, black_border, ndim):
    """the definition: the distance of a voxel to the nearest voxel of another value -- or, with black_border, to the outside of the
    array along the first ndim axes -- measured between centres, a voxel outside lying one pitch behind the face"""
    import scipy.ndimage as ndi
    pad = [(1, 1) if (black_border and a < ndim) else (0, 0) for a in range(3)]
    out = np.zeros(lab.shape, dtype=f64)
    for v in np.unique(lab[lab != 0]).tolist():
        inside = np.pad(lab == v, pad, constant_values=False)
        if inside.all():
            d = np.full(inside.shape, np.inf)
        else:
            d = ndi.distance_transform_edt(inside, sampling=an)
        core = d[tuple(slice(p[0], d.shape[a] - p[1]) for a, p in enumerate(pad))]
        out[lab == v] = core[lab == v]
    return out


def assert_edt(lab, an, black_border, ndim, plain=False):
    lab = fortran(lab)
    out = NR.canary(lab.size, f32, lab.shape)
    args = [lab, lab.itemsize] + ([] if plain else [ndim]) + [*lab.shape, float(an[0]), float(an[1]), float(an[2]), int(black_border), out]
    rc, after = both(ORACLE, "ko_edt" if plain else "ko_edt_nd", args)
    assert rc == 0
    np.testing.assert_allclose(after(out), edt_by_scipy(lab, an, black_border, ndim), rtol=1e-6)


@functools.lru_cache(maxsize=None)
def edt_labels():
    lab = shapes.voronoi_labels(SHAPE, 6, 11).astype(np.int64) - 1000 + 1            # 1..6
    lab[np.random.default_rng(37).random(SHAPE) < 0.1] = 0
    return lab


@replays("ko_edt_nd", "ko_edt")
@pytest.mark.parametrize("dtype", [u8, u16, u32, u64])
def test_oracle_edt(dtype):
    lab = edt_labels().astype(dtype) * dtype(int(np.iinfo(dtype).max) // 6)       # values that need the whole word
    for an in ANISOTROPIES:
        for black_border in (0, 1):
            assert_edt(lab, an, black_border, 3)
    assert_edt(lab, (16, 16, 40), 1, 3, plain=True)
    # extent-1 axes, as axes of the array and as axes that do not exist; one voxel
    for sub, ndim in ((lab[:, :, 5:6], 3), (lab[:, :, 5:6], 2), (lab[:, 7:8, 5:6], 1), (lab[:, 7:8, :], 3), (lab[3:4, :, :], 3),
                      (lab[:1, :1, :1] * 0 + 1, 3), (lab[:1, :1, :1] * 0 + 1, 1), (lab[:1, :1, :1] * 0, 3)):
        for black_border in (0, 1):
            assert_edt(sub.copy(), (16, 16, 40), black_border, ndim)


@replays("ko_edt_nd")
def test_oracle_edt_refuses_three_byte_labels():
    out = NR.canary(24, f32)
    rc, after = both(ORACLE, "ko_edt_nd", [np.ones(72, dtype=u8), 3, 3, 4, 3, 2, 1.0, 1.0, 1.0, 0, out])
    assert rc == 1 and NR.is_canary(after(out))


# ---- the oracle: distance field from a source ------------------------------------------------------------------------------------

def edf(mask, source, an, radius=0.0, graph=None):
    mask = fortran(mask, u8)
    out, max_loc, max_val = NR.canary(mask.size, f32, mask.shape), NR.canary(1, u64), NR.canary(1, f32)
    search = ("ko_edf", [mask, *mask.shape, float(an[0]), float(an[1]), float(an[2]), int(source), float(radius), out, max_loc, max_val])
    calls = [search] if graph is None else [("ko_set_voxel_graph", [graph]), search, ("ko_set_voxel_graph", [None])]
    rets, after = both_many(ORACLE, calls)
    return rets[len(calls) // 2], after(out), after(max_loc), after(max_val)


@replays("ko_edf", "ko_set_voxel_graph")
def test_oracle_edf():
    mask = tube()
    inside, outside = np.flatnonzero(mask.ravel(order="F")), np.flatnonzero(mask.ravel(order="F") == 0)
    for an in ANISOTROPIES:
        plain = None
        for radius in (0.0, 3.0 * an[0]):
            rc, out, max_loc, max_val = edf(mask, inside[0], an, radius)
            flat, reached = out.ravel(order="F"), np.isfinite(out)
            assert rc == 0 and flat[inside[0]] == 0 and not reached[mask == 0].any() and reached.sum() > inside.size // 2
            assert max_val[0] == out[reached].max() and int(max_loc[0]) == np.flatnonzero(flat == max_val[0])[0]   # ties: smallest index
            plain = out if plain is None else plain
        # with a voxel graph set for the call, then cleared: fewer steps allowed, no distance gets shorter
        rc, out, _, _ = edf(mask, inside[0], an, graph=random_graph(SHAPE, 41))
        assert rc == 0 and np.all(out >= plain) and np.any(out > plain)
        rc, again, _, _ = edf(mask, inside[0], an)
        assert np.array_equal(again, plain)
        # a source on background, a source outside the volume: KO_EINVAL, the field is +inf, the maximum is not reported
        for source in (outside[0], mask.size):
            rc, out, max_loc, max_val = edf(mask, source, an)
            assert rc == 1 and np.all(out == np.inf) and NR.is_canary(max_loc) and NR.is_canary(max_val)
    # extent-1 axes, one voxel
    px, py, pz = tube_centre()
    for sub in (mask[:, :, pz:pz + 1], mask[:, py:py + 1, pz:pz + 1], mask[px:px + 1, :, :]):
        sub = fortran(sub.copy())
        rc, out, _, _ = edf(sub, np.flatnonzero(sub.ravel(order="F"))[0], (16, 16, 40))
        assert rc == 0 and np.all(out[sub == 0] == np.inf)
    rc, out, max_loc, max_val = edf(np.ones((1, 1, 1), dtype=u8), 0, (16, 16, 40), graph=np.zeros((1, 1, 1), dtype=u32))
    assert rc == 0 and out.tolist() == [[[0.0]]] and max_loc.tolist() == [0] and max_val.tolist() == [0.0]


# ---- the oracle: PDRF and the target order ----------------------------------------------------------------------------------------

@replays("ko_pdrf")
def test_oracle_pdrf_golden():
    z = np.load(os.path.join(G, "pdrf.npz"))
    for i in range(int(z["n"])):
        dbf, daf = z["dbf_%d" % i].astype(f32), z["daf_in_%d" % i].astype(f32)
        dbf_max, scale, expo, max_daf = z["par_%d" % i]
        M = f32(1 / (f32(dbf_max) ** 1.01))                                         # oracle.compute_pdrf's
        out = NR.canary(dbf.size, f32)
        rc, after = both(ORACLE, "ko_pdrf", [dbf, daf, dbf.size, float(M), int(expo), float(f32(scale)), float(f32(max_daf)), out])
        assert rc == 0 and np.array_equal(after(daf), z["daf_out_%d" % i]), i       # DAF is mutated
        if int(expo) & (int(expo) - 1) == 0:                                        # (the powf branch is the host libm's: not pinned)
            assert np.array_equal(after(out), z["out_%d" % i]), i
    out = NR.canary(0, f32)
    rc, _ = both(ORACLE, "ko_pdrf", [np.zeros(0, dtype=f32), np.zeros(0, dtype=f32), 0, 0.5, 16, 1e5, 2.0, out])
    assert rc == 0


@replays("ko_target_order")
def test_oracle_target_order():
    cases = []
    z = np.load(os.path.join(G, "target_finder.npz"))
    for i in range(int(z["n"])):
        shape = tuple(z["shape_%d" % i])
        cases.append((unpack(z["mask_%d" % i], shape), fortran(z["daf_%d" % i].reshape(shape, order="F"))))
    z = np.load(os.path.join(G, "legacy_targets.npz"))
    for i in range(0, int(z["n"]), 3):
        shape = tuple(int(v) for v in z["shape_%d" % i])
        cases.append((unpack(z["mask_%d" % i], shape), fortran(z["field_%d" % i].reshape(shape, order="F"))))
    cases.append((tube(), fortran(np.random.default_rng(43).integers(0, 4, SHAPE).astype(f32))))       # many equal keys
    cases.append((np.zeros((3, 2, 2), dtype=u8, order="F"), np.ones((3, 2, 2), dtype=f32, order="F")))  # nothing to order
    for mask, daf in cases:
        idx = np.flatnonzero(mask.ravel(order="F"))
        order = NR.canary(idx.size, u32)
        n, after = both(ORACLE, "ko_target_order", [mask, daf, mask.size, order])
        want = idx[np.argsort(daf.ravel(order="F")[idx], kind="stable")][::-1]       # descending key, ties by descending index
        assert n == idx.size and np.array_equal(after(order), want)


# ---- the oracle: the searches over a weight field ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def weight_field():
    """a PDRF-like field on the tube: +inf outside, weights in [1, 2) inside, three rail voxels of weight 0 at its low end"""
    mask = tube()
    f = np.full(SHAPE, np.inf, dtype=f32, order="F")
    f[mask != 0] = (1 + np.random.default_rng(47).random(int(mask.sum()))).astype(f32)
    inside = np.flatnonzero(mask.ravel(order="F"))
    flat = f.reshape(-1, order="F")
    flat[inside[:3]] = 0
    f.setflags(write=False)
    return f, inside, np.flatnonzero(mask.ravel(order="F") == 0)


def field_cases(rails=True):
    """(name, field, a source, another voxel of the object, a wall voxel); rails=False: the rails get an ordinary weight (the
    parental field has no rails: zero weights make plateaus that a parent pointer cannot express)"""
    f, inside, outside = weight_field()
    if not rails:
        f = fortran(np.where(f == 0, f32(1.5), f))
    px, py, pz = tube_centre()
    yield "tube", f, int(inside[-1]), int(inside[len(inside) // 2]), int(outside[0])
    for name, sub in (("one layer", f[:, :, pz:pz + 1]), ("one column", f[px:px + 1, :, :]), ("one row", f[:, py:py + 1, pz:pz + 1])):
        sub = fortran(sub.copy())
        ok = np.flatnonzero(np.isfinite(sub.ravel(order="F")))
        yield name, sub, int(ok[-1]), int(ok[0]), int(np.flatnonzero(~np.isfinite(sub.ravel(order="F")))[0])


@replays("ko_railroad")
def test_oracle_railroad():
    import oracle
    for name, f, source, other, wall in field_cases():
        n = f.size
        for target in (source, other):
            d, path, npath, settled = NR.canary(n, f32, f.shape), NR.canary(n, u64), NR.canary(1, i64), NR.canary(1, i64)
            rc, after = both(ORACLE, "ko_railroad", [f, *f.shape, target, d, path, npath, settled])
            if not (f == 0).any():                                               # a slice without a rail: KO_ENOPATH
                assert rc == 3, name
                continue
            k = int(after(npath)[0])
            assert rc == 0 and 1 <= k <= n and int(after(path)[k - 1]) == target and NR.is_canary(after(path)[k:]), name
            assert f.ravel(order="F")[int(after(path)[0])] == 0                  # rail end first
            assert np.array_equal(oracle.locs_to_pts(after(path)[:k], f.shape), oracle.railroad(f, oracle.pt_of(target, f.shape)))
        # a target on a wall or outside the volume: KO_EINVAL, nothing is written; a target that is a rail: itself
        for target in (wall, n):
            d, path, npath, settled = NR.canary(n, f32), NR.canary(n, u64), NR.canary(1, i64), NR.canary(1, i64)
            rc, after = both(ORACLE, "ko_railroad", [f, *f.shape, target, d, path, npath, settled])
            assert rc == 1 and all(NR.is_canary(after(a)) for a in (d, path, npath, settled)), name
    f, inside, _ = weight_field()
    d, path, npath = NR.canary(f.size, f32), NR.canary(f.size, u64), NR.canary(1, i64)
    rc, after = both(ORACLE, "ko_railroad", [f, *f.shape, int(inside[0]), d, path, npath, None])
    assert rc == 0 and after(npath).tolist() == [1] and int(after(path)[0]) == inside[0] and NR.is_canary(after(d))
    one = np.ones((1, 1, 1), dtype=f32)
    rc, _ = both(ORACLE, "ko_railroad", [one, 1, 1, 1, 0, NR.canary(1, f32), NR.canary(1, u64), NR.canary(1, i64), NR.canary(1, i64)])
    assert rc == 3


@replays("ko_field_distances", "ko_parental_field", "ko_path_from_parents", "ko_path_to_source", "ko_set_voxel_graph")
def test_oracle_parental_searches():
    for name, f, source, target, wall in field_cases(rails=False):
        n = f.size
        d = NR.canary(n, f32, f.shape)
        rc, after = both(ORACLE, "ko_field_distances", [f, *f.shape, source, d])
        dist = after(d)
        assert rc == 0 and dist.ravel(order="F")[source] == 0, name
        d2, parents = NR.canary(n, f32, f.shape), NR.canary(n, u32, f.shape)
        rc, after = both(ORACLE, "ko_parental_field", [f, *f.shape, source, d2, parents])
        par = after(parents)
        assert rc == 0 and np.array_equal(after(d2), dist) and par.ravel(order="F")[source] == 0, name
        assert np.array_equal(par != 0, np.isfinite(dist) & (np.arange(n).reshape(f.shape, order="F") != source)), name
        reachable = np.isfinite(dist.ravel(order="F")[target])
        path, npath = NR.canary(n, u64), NR.canary(1, i64)
        rc, after = both(ORACLE, "ko_path_from_parents", [par, n, target, path, npath])
        k = int(after(npath)[0])
        by_parents = after(path)[:k]
        assert rc == 0 and by_parents[-1] == target and NR.is_canary(after(path)[k:]), name
        path, npath = NR.canary(n, u64), NR.canary(1, i64)
        rc, after = both(ORACLE, "ko_path_to_source", [f, dist, *f.shape, source, target, path, npath])
        if reachable:
            assert rc == 0 and by_parents[0] == source
            assert np.array_equal(after(path)[:int(after(npath)[0])], by_parents), name       # both follow the canonical predecessor
        else:
            assert rc == 3 and NR.is_canary(after(path)) and NR.is_canary(after(npath)), name
        # with a voxel graph (one-way edges: the predecessor rule reads the neighbour's word), set and cleared around the search
        graph = random_graph(f.shape, 53)
        d3, parents3 = NR.canary(n, f32, f.shape), NR.canary(n, u32, f.shape)
        rets, after = both_many(ORACLE, [("ko_set_voxel_graph", [graph]), ("ko_parental_field", [f, *f.shape, source, d3, parents3]),
                                         ("ko_set_voxel_graph", [None])])
        assert rets[1] in (0, 4) and np.all(after(d3) >= dist), name
        # a source on a wall or outside the volume: KO_EINVAL, nothing is written
        for bad in (wall, n):
            d4, parents4 = NR.canary(n, f32), NR.canary(n, u32)
            rc, after = both(ORACLE, "ko_field_distances", [f, *f.shape, bad, d4])
            assert rc == 1 and NR.is_canary(after(d4)), name
            rc, after = both(ORACLE, "ko_parental_field", [f, *f.shape, bad, d4, parents4])
            assert rc == 1 and NR.is_canary(after(d4)) and NR.is_canary(after(parents4)), name
    one = np.ones((1, 1, 1), dtype=f32)
    d, parents = NR.canary(1, f32), NR.canary(1, u32)
    rc, after = both(ORACLE, "ko_parental_field", [one, 1, 1, 1, 0, d, parents])
    assert rc == 0 and after(d).tolist() == [0] and after(parents).tolist() == [0]


# ---- the oracle: invalidation -----------------------------------------------------------------------------------------------------

def invalidate_ball(mask, dbf, path_pts, scale, const, an, graph=None):
    """oracle.roll_invalidation_ball_inside_component through the replay: the radii, then the flood -> (count, mask after)"""
    mask, dbf = fortran(mask, u8), fortran(dbf, f32)
    locs = lin(path_pts, mask.shape)
    radii = NR.canary(locs.size, f32)
    _, after = both(ORACLE, "ko_ball_radii", [dbf, locs, locs.size, float(f32(scale)), float(f32(const)), radii])
    radii = after(radii)
    t = f32(scale) * dbf.ravel(order="F")[locs.astype(i64)]
    assert np.array_equal(radii, t + f32(const))
    count, ops = NR.canary(1, i64), NR.canary(1, i64)
    head = [mask, *mask.shape, float(an[0]), float(an[1]), float(an[2]), locs, radii, locs.size]
    if graph is None:
        rc, after = both(ORACLE, "ko_invalidate_ball", head + [count, ops])
    else:
        rc, after = both(ORACLE, "ko_invalidate_ball_graph", head + [fortran(graph, u32), count, ops])
    assert rc == 0
    return int(after(count)[0]), after(mask)


def golden_flood(z, i):
    shape = tuple(int(v) for v in z["shape_%d" % i])
    path = z["path_%d" % i]
    dbf = np.zeros(shape, dtype=f32, order="F")
    dbf[path[:, 0], path[:, 1], path[:, 2]] = z["dbfpath_%d" % i]
    scale, const = z["sc_%d" % i]
    return shape, unpack(z["mask_%d" % i], shape), path, dbf, scale, const, z["an_%d" % i]


@replays("ko_invalidate_ball", "ko_ball_radii")
def test_oracle_invalidate_ball():
    import oracle
    z = np.load(os.path.join(G, "invalidation_ball.npz"))
    for i in range(int(z["n"])):
        shape, mask, path, dbf, scale, const, an = golden_flood(z, i)
        count, out = invalidate_ball(mask, dbf, path, scale, const, an)
        assert count == int(z["count_%d" % i]) and np.array_equal(out, unpack(z["after_%d" % i], shape)), i
    mask = tube()
    pts = oracle.locs_to_pts(np.flatnonzero(mask.ravel(order="F"))[::97], SHAPE)
    for an in ANISOTROPIES:
        dbf = oracle.edt(mask, an)
        count, out = invalidate_ball(mask, dbf, pts, 1.5, 2.0 * an[0], an)
        assert 0 < count == int(mask.sum()) - int(out.sum()) and np.all(out <= mask)
        count, out = invalidate_ball(mask, dbf, np.zeros((0, 3), dtype=i64), 1.5, 2.0, an)         # no source: nothing happens
        assert count == 0 and np.array_equal(out, mask)
    px, py, pz = tube_centre()
    for sub in (mask[:, :, pz:pz + 1], mask[px:px + 1, :, :], np.ones((1, 1, 1), dtype=u8)):        # extent-1 axes, one voxel
        sub = fortran(sub.copy())
        first = oracle.locs_to_pts(np.flatnonzero(sub.ravel(order="F"))[:1], sub.shape)
        count, out = invalidate_ball(sub, np.full(sub.shape, 2.0, dtype=f32), first, 1.0, 0.5, (16, 16, 40))
        assert count >= 1 and count == int(sub.sum()) - int(out.sum())


@replays("ko_invalidate_ball_graph", "ko_ball_radii")
def test_oracle_invalidate_ball_graph():
    import oracle
    z = np.load(os.path.join(G, "invalidation_ball_graph.npz"))
    for i in range(int(z["n"])):
        shape, mask, path, dbf, scale, const, an = golden_flood(z, i)
        graph = z["graph_%d" % i].reshape(shape, order="F")
        count, out = invalidate_ball(mask, dbf, path, scale, const, an, graph=graph)
        assert count == int(z["count_%d" % i]) and np.array_equal(out, unpack(z["after_%d" % i], shape)), i
    mask = tube()
    pts = oracle.locs_to_pts(np.flatnonzero(mask.ravel(order="F"))[::97], SHAPE)
    for an in ANISOTROPIES:
        dbf = oracle.edt(mask, an)
        free, _ = invalidate_ball(mask, dbf, pts, 1.5, 2.0 * an[0], an)
        count, out = invalidate_ball(mask, dbf, pts, 1.5, 2.0 * an[0], an, graph=random_graph(SHAPE, 59, keep=0.6))
        assert 0 < count <= free and count == int(mask.sum()) - int(out.sum())
        count, out = invalidate_ball(mask, dbf, np.zeros((0, 3), dtype=i64), 1.5, 2.0, an, graph=random_graph(SHAPE, 59))
        assert count == 0 and np.array_equal(out, mask)


@replays("ko_invalidate_cube")
def test_oracle_invalidate_cube():
    import oracle

    def cube(mask, dbf, path_pts, scale, const, an):
        mask, dbf = fortran(mask, u8), fortran(dbf, f32)
        locs, count = lin(path_pts, mask.shape), NR.canary(1, i64)
        rc, after = both(ORACLE, "ko_invalidate_cube", [mask, dbf, *mask.shape, float(an[0]), float(an[1]), float(an[2]), locs, locs.size,
                                                        float(f32(scale)), float(f32(const)), count])
        assert rc == 0
        return int(after(count)[0]), after(mask)

    z = np.load(os.path.join(G, "invalidation_cube.npz"))
    for i in range(int(z["n"])):
        shape, mask, path, dbf, scale, const, an = golden_flood(z, i)
        count, out = cube(mask, dbf, path, scale, const, an)
        assert count == int(z["count_%d" % i]) and np.array_equal(out, unpack(z["after_%d" % i], shape)), i
    # the counts the reference asserts (tests/test_oracle_golden.py), cubes that reach over every face
    assert cube(np.ones((10, 10, 10)), np.zeros((10, 10, 10)), [(5, 5, 5)], 0.0, 2.0, (1, 1, 1))[0] == 125
    assert cube(np.ones((3, 4, 5)), np.zeros((3, 4, 5)), [(2, 3, 4)], 0.0, 1.0, (1, 1, 1))[0] == 8
    assert cube(np.ones((13, 17, 14)), np.zeros((13, 17, 14)), [(1, 16, 0)], 0.0, 0.965, (0.94, 0.93, 2.58))[0] == 9
    mask = tube()
    pts = oracle.locs_to_pts(np.flatnonzero(mask.ravel(order="F"))[::97], SHAPE)
    for an in ANISOTROPIES:
        count, out = cube(mask, oracle.edt(mask, an), pts, 1.5, 2.0 * an[0], an)
        assert 0 < count == int(mask.sum()) - int(out.sum())
        assert cube(mask, oracle.edt(mask, an), np.zeros((0, 3), dtype=i64), 1.5, 2.0, an)[0] == 0
    assert cube(np.ones((1, 1, 1)), np.full((1, 1, 1), 40.0), [(0, 0, 0)], 1.0, 0.0, (16, 16, 40))[0] == 1


# ---- completeness -----------------------------------------------------------------------------------------------------------------

def test_every_symbol_has_a_case():
    """the programs know exactly the host entry points of the ABI and the oracle functions oracle/__init__.py binds, and every one
    of them is replayed by a test of this module"""
    from kimimaro_amd import _abi
    host = {s for s in _abi.SYMBOLS if s.startswith("kh_host_")}
    with open(os.path.join(os.path.dirname(HERE), "oracle", "__init__.py")) as f:
        bound = set(re.findall(r"\bL\.(ko_\w+)\.argtypes", f.read()))
    assert len(host) == 8 and len(bound) == 20
    assert set(NR.known_functions(HOST)) - {"selftest_overrun"} == host
    assert set(NR.known_functions(ORACLE)) - {"selftest_overrun"} == bound
    assert {f for f, tests in CASES.items() if tests} == host | bound


def test_report_timings(capsys):
    """prints what the build and the child processes cost so far (figures for the log; nothing is asserted on them)"""
    build, run, children = NR.timings()
    with capsys.disabled():
        print("\nnative replay: build %.1f s, %d child processes %.1f s" % (build or 0.0, children, run))
