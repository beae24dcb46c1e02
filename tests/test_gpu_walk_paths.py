"""kh_walk_orient and kh_walk_emit against tests/walk_paths_ref.py, and what is built on them against the host functions they
stand for: paths_many = Skeleton.paths, utility._xs_occurrences_many = utility._xs_occurrences bit for bit, and the section functions
with walk="device" = the same with walk="host".

The entry points are also called directly with buffers sized as kimimaro_amd.forest sizes them, every byte 0xA5 and 64 elements more
than the call owns: afterwards every table equals the statement's, grown from the same sentinel, and the 64 still hold it."""
import copy

import numpy as np
import pytest

import walk_paths_ref as W

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64
PATH_CASES = W.path_cases()
OCC_CASES = W.occurrence_cases()


class Guarded:
    """a device buffer of n elements of `dtype` and GUARD more behind them, every byte FILL"""

    def __init__(self, eng, n, dtype):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.t = eng.torch.full(((self.n + GUARD) * self.dtype.itemsize,), FILL, dtype=eng.torch.uint8, device=eng.device)
        self.ptr = eng.ptr(self.t)

    def down(self):
        """the n elements, once the GUARD behind them is seen to be untouched"""
        host = self.t.cpu().numpy()
        assert np.all(host[self.n * self.dtype.itemsize:] == FILL), "the call wrote behind its %d elements" % self.n
        return host[:self.n * self.dtype.itemsize].view(self.dtype).copy()


def up(eng, a):
    a = np.ascontiguousarray(a).reshape(-1)
    return eng.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(eng.device)


# ---- 1. the device calls, table for table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_the_tables_of_both_calls(name):
    from kimimaro_amd import _abi, forest, ops
    eng = ops.engine()
    w = forest.Walk(PATH_CASES[name])
    n, ns, m = w.nverts, int(w.nbr.size), int(w.edges.shape[0])
    comp = W.labels(w.edges, n)
    T = forest.WalkTables(w, comp)
    nc, k, npaths = int(T.crit.size), int(T.root.size), T.npaths
    assert k >= 1 and npaths >= 1
    # kh_forest_components, then kh_walk_orient
    g_comp = Guarded(eng, n, np.uint32)
    d_edges = up(eng, w.edges)
    _abi.check(eng.lib.kh_forest_components(eng.ptr(d_edges), n, m, g_comp.ptr, eng.stream()))
    d_in = [up(eng, a) for a in (w.row_start, w.nbr, T.crit, T.crit_start, T.leaf_start)]
    g = {"slots": Guarded(eng, 3 * ns, np.uint32), "recs": Guarded(eng, 8 * nc, np.uint32)}
    g.update({key: Guarded(eng, n, np.uint32) for key in ("parent", "depth")})
    g.update({key: Guarded(eng, npaths, np.uint32) for key in ("path_leaf", "path_len")})
    _abi.check(eng.lib.kh_walk_orient(eng.ptr(d_in[0]), eng.ptr(d_in[1]), g_comp.ptr, eng.ptr(d_in[2]), eng.ptr(d_in[3]), eng.ptr(d_in[4]),
                                      n, ns, nc, k, npaths, g["slots"].ptr, g["recs"].ptr, g["parent"].ptr, g["depth"].ptr,
                                      g["path_leaf"].ptr, g["path_len"].ptr, eng.stream()))
    eng.sync()
    assert np.array_equal(g_comp.down(), comp)
    want = W.orient_tables(w, comp, T, fill=FILL)
    got = {key: buf.down() for key, buf in g.items()}
    for key in ("parent", "depth", "path_leaf", "path_len"):
        assert np.array_equal(got[key], getattr(want, key)), key
    for j, key in enumerate(W.Tables.SLOT):
        assert np.array_equal(got["slots"][j * ns:(j + 1) * ns], getattr(want, key)), key
    for j, key in enumerate(W.Tables.RECORD):
        assert np.array_equal(got["recs"][j * nc:(j + 1) * nc], getattr(want, key)), key
    # kh_walk_emit: the paths alone, then with the normals of both regimes
    pstart = np.concatenate([[0], np.cumsum(want.path_len.astype(np.int64))]).astype(np.int64)
    nocc = int(pstart[-1])
    vox = np.round(np.concatenate([np.asarray(s.vertices).reshape(-1, 3) for s in PATH_CASES[name]])).astype(np.int32)
    d_pstart, d_vox = eng.torch.from_numpy(pstart).to(eng.device), eng.torch.from_numpy(vox.reshape(-1)).to(eng.device)
    word = np.full(1, FILL, dtype=np.uint8)
    for window in (0, 1, 3):
        e = {"occ": Guarded(eng, nocc, np.uint32), "normal": Guarded(eng, 3 * nocc, np.float64), "first": Guarded(eng, 3 * nocc, np.float64)}
        _abi.check(eng.lib.kh_walk_emit(g["parent"].ptr, g["path_leaf"].ptr, eng.ptr(d_pstart), eng.ptr(d_vox), n, npaths, nocc, window,
                                        e["occ"].ptr, e["normal"].ptr, e["first"].ptr, eng.stream()))
        eng.sync()
        occ, normal, first = W.emit_tables(want.parent, want.path_leaf, pstart, vox, window, fill=FILL)
        assert np.array_equal(e["occ"].down(), occ), window
        got_normal, got_first = e["normal"].down(), e["first"].down()
        if window == 0:
            assert np.all(got_normal.view(np.uint8) == word)
        else:
            assert np.array_equal(W.bits(got_normal.reshape(-1, 3)), W.bits(normal)), window
        if window <= 1:
            assert np.all(got_first.view(np.uint8) == word)
        else:
            assert np.array_equal(got_first.view(np.uint64), first.reshape(-1).view(np.uint64)), window


# ---- 2. the public walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_paths_many_is_skeleton_paths(name):
    import kimimaro_amd
    from kimimaro_amd import ops
    skels = PATH_CASES[name]
    want = [s.paths(return_indices=True) for s in skels]
    stats = {}
    got = kimimaro_amd.paths_many(skels, stats=stats)
    assert len(got) == len(skels) and all(W.same_paths(g, w) for g, w in zip(got, want))
    assert stats["walk_host"] == (0 if name in W.TREE_CASES else 1)
    assert all(W.same_paths(g, s.paths()) for g, s in zip(kimimaro_amd.paths_many(skels, return_indices=False), skels))
    assert all(W.same_paths(ops.skeleton_paths(s), w) for s, w in zip(skels, want))


@pytest.mark.parametrize("name", sorted(OCC_CASES))
def test_occurrences_many_is_xs_occurrences(name):
    from kimimaro_amd import ops, utility
    jobs, an, shape, windows, steps = OCC_CASES[name]
    for window in windows:
        for step in steps:
            stats = {}
            got = utility._xs_occurrences_many(ops.engine(), jobs, an, shape, window, step, stats)
            assert len(got) == len(jobs)
            for (gv, go, gn, gb), (skel, _, offset) in zip(got, jobs):
                wv, wo, wn = utility._xs_occurrences(skel, an, offset, shape, window, step)
                assert gv.dtype == wv.dtype and np.array_equal(gv, wv), (window, step)
                assert go.dtype == wo.dtype and np.array_equal(go, wo), (window, step)
                assert gn.dtype == wn.dtype and gn.shape == wn.shape and np.array_equal(W.bits(gn), W.bits(wn)), (window, step)
                assert np.array_equal(np.flatnonzero(gb), skel.branches())
            assert stats["walk_host"] == (1 if name == "cyclic_between" else 0)


# ---- 3. the sections: walk="device" against walk="host" -----------------------------------------------------------------------------------
def tubes(nx):
    """(labels u32 [nx, 48, 48], {label: Skeleton}): a tube along x that spans the volume, one along y, and a forked one (a trunk
    along z with a side branch along x)"""
    from kimimaro_amd import Skeleton
    lab = np.zeros((nx, 48, 48), dtype=np.uint32, order="F")
    x, y, z = np.meshgrid(np.arange(nx), np.arange(48), np.arange(48), indexing="ij")
    lab[((y - 12) ** 2 + (z - 12) ** 2 <= 9) & (x >= 4) & (x <= nx - 5)] = 1
    lab[((x - 36) ** 2 + (z - 34) ** 2 <= 4) & (y >= 4) & (y <= 43)] = 2
    lab[((x - 14) ** 2 + (y - 34) ** 2 <= 9) & (z >= 4) & (z <= 44)] = 3
    lab[((y - 34) ** 2 + (z - 24) ** 2 <= 4) & (x >= 14) & (x <= 30)] = 3
    chain = lambda pts: (np.array(pts, dtype=np.float32), np.array([[k, k + 1] for k in range(len(pts) - 1)], dtype=np.uint32))
    a = Skeleton(*chain([[k, 12, 12] for k in range(4, nx - 4)]), segid=1)
    b = Skeleton(*chain([[36, k, 34] for k in range(4, 44)]), segid=2)
    trunk, edges = chain([[14, 34, k] for k in range(4, 45)])
    side = np.array([[k, 34, 24] for k in range(15, 31)], dtype=np.float32)
    at = 41 + np.arange(side.shape[0])
    side_edges = np.stack([np.concatenate([[20], at[:-1]]), at], axis=1).astype(np.uint32)
    c = Skeleton(np.concatenate([trunk, side]), np.concatenate([edges, side_edges]), segid=3)
    return lab, {1: a, 2: b, 3: c}


_CACHE = {}


def small():
    if "small" not in _CACHE:
        lab, skels = tubes(48)
        _CACHE["small"] = (lab, skels, run("plain", lab, copy.deepcopy(skels), {}))
    return _CACHE["small"]


def run(which, lab, skels, kw):
    import kimimaro_amd
    if which == "single":
        kimimaro_amd.cross_sectional_area_single(lab == 3, skels[3], **kw)
        return skels
    fn = kimimaro_amd.cross_sectional_area_filled if which == "filled" else kimimaro_amd.cross_sectional_area
    return fn(lab, skels, **kw)


def assert_same_attributes(got, want):
    assert list(got) == list(want)
    for key in want:
        a, b = got[key], want[key]
        if not hasattr(b, "cross_sectional_area"):
            assert not hasattr(a, "cross_sectional_area")
            continue
        assert a.cross_sectional_area.dtype == np.float32 and a.cross_sectional_area_contacts.dtype == np.uint8
        assert a.cross_sectional_area.tobytes() == b.cross_sectional_area.tobytes(), key
        assert np.array_equal(a.cross_sectional_area_contacts, b.cross_sectional_area_contacts), key
        assert a.extra_attributes == b.extra_attributes


@pytest.mark.parametrize("which", ["plain", "filled", "single"])
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("smoothing_window", [1, 3])
def test_sections_with_the_device_walk_equal_the_host_walk(smoothing_window, step, which):
    lab, skels, before = small()
    assert sum(int((s.cross_sectional_area > 0).sum()) for s in before.values()) > 100
    for repair_contacts in (False, True):
        for multipass in (False, True):
            kw = dict(smoothing_window=smoothing_window, step=step, repair_contacts=repair_contacts, multipass=multipass)
            start = before if (repair_contacts or multipass) else skels       # with values from an earlier pass, or without any
            stats = {}
            host = run(which, lab, copy.deepcopy(start), dict(kw, walk="host"))
            device = run(which, lab, copy.deepcopy(start), dict(kw, walk="device", _stats=stats))
            assert_same_attributes(device, host)
            assert stats["walk_host"] == 0 and stats["paths"] == (2 if which == "single" else 4) and stats["walk_s"] > 0
            assert int((device[3].cross_sectional_area > 0).sum()) > 20


def test_chunked_sections_with_the_device_walk():
    import kimimaro_amd
    lab, skels = tubes(64)
    for kw in (dict(smoothing_window=1, step=1), dict(smoothing_window=3, step=3)):
        want = kimimaro_amd.cross_sectional_area(lab, copy.deepcopy(skels), **kw)
        mine, timings = copy.deepcopy(skels), {}
        out = kimimaro_amd.cross_sectional_area_chunked(lab, mine, chunk_shape=(32, 48, 48), halo=8, timings=timings, walk="device", **kw)
        assert out is mine and timings["cores"] == 2 and timings["walk_host"] == 0 and timings["paths"] == 4
        assert_same_attributes(mine, want)
        assert not any(np.any(s.cross_sectional_area_contacts & 64) for s in mine.values())
        evaluated = sum(int((s.cross_sectional_area > 0).sum()) for s in mine.values())       # every step-th vertex and the ends
        assert evaluated > sum(len(s.vertices) for s in mine.values()) // (kw["step"] + 1)
