"""The flood of csrc/heap.h (invalidate_ball<PROF, H>) in all four forms it is compiled in -- Heap<1> and Heap<2>, plain and profiled.

First alone: kh_heap_flood makes ONE call of it by one wave on inputs whose regime tests/test_heap_flood_host.py proves from the
oracle's peak heap size: on Heap<2> (8 191 slots in LDS) a heap that never leaves LDS, one whose new leaves go to memory under
parents in LDS (peak between 8 191 and 16 383) and one whose batched append reads parents from memory (peak above 16 383), each
without and with a voxel graph; the count, the mask, the status and the pushes against the oracle, the heap's memory against a
sentinel, and the capacity edge (capacity = peak and peak - 1) with guard nodes behind the buffer.

Then inside the path kernel: one small volume whose large label -- the (40, 32, 20) block -- has a first flood that peaks at 16 976
nodes and leaves 2 183 voxels for eight more (scale 0.5, const 10: flood_cases.PATH_SCALE says why, the host test asserts the
peak), through every engine knob no other test sets: the big LDS heap on and off, the profiled build, heap_prio, big_threads, and
big_lds_labels with one wave per label.  Every variant must give the oracle's skeletons and, per label, the oracle's pushes.

What notices a wrong key select in the append is mostly the push count: a heap out of order pops a voxel's nodes in another order,
the flood pushes a few nodes more or fewer, and the mask often ends the same (measured with two scratch builds, BENCH_NOTES.md)."""
import numpy as np
import pytest

import flood_cases as FC

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD_NODES = 64
GUARD_WORDS = 16
TOP = {1: 127, 2: 8191}
ST_HEAP_OVERFLOW = 2          # KH_ST_HEAP_OVERFLOW
BUILDS = [(1, 0), (1, 1), (2, 0), (2, 1)]         # (topl, profile)


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


_device_inputs = {}


def device_inputs(eng, c):
    """the case's read-only device arrays, made once: neighbour masks (through the graph, if any), corner gate, DBF, path"""
    key = (c.row, c.radii)
    if key not in _device_inputs:
        from kimimaro_amd import _abi
        t, P = eng.torch, eng.ptr
        sx, sy, sz = c.shape
        nvox = sx * sy * sz
        d_cc = t.ones(nvox, dtype=t.int32, device=eng.device)
        d_nbr = eng.empty(nvox, t.int32)
        _abi.check(eng.lib.kh_neighbor_mask(P(d_cc), 4, sx, sy, sz, P(d_nbr), eng.stream()))
        d_gate = None
        if c.graph is not None:
            d_graph = eng.graph_to_device(np.array(c.graph), c.shape)
            d_gate = t.zeros(nvox + 4, dtype=t.uint8, device=eng.device)
            _abi.check(eng.lib.kh_apply_voxel_graph(P(d_nbr), P(d_graph), nvox, P(d_gate), eng.stream()))
        locs = np.array([x + sx * (y + sy * z) for x, y, z in c.path], dtype=np.uint32)
        assert int(locs.max()) < nvox
        _device_inputs[key] = (d_nbr, d_gate, eng.to_device(np.array(c.dbf)), t.from_numpy(locs.view(np.int32).copy()).to(eng.device))
    return _device_inputs[key]


def run_flood(eng, c, topl, profile, capacity=None):
    """one kh_heap_flood on a mask of ones -> (count, pushes, status, cyc3 [3], mask after, node buffer [allocated + guard, 4]);
    the buffers are sentinel filled and what lies behind the words the entry writes is checked here"""
    from kimimaro_amd import _abi
    t, P = eng.torch, eng.ptr
    d_nbr, d_gate, d_dbf, d_path = device_inputs(eng, c)
    sx, sy, sz = c.shape
    nvox = sx * sy * sz
    capacity = c.peak + 64 if capacity is None else capacity
    allocated = max(capacity, TOP[topl] + 1)
    d_alive = t.ones(nvox + GUARD_WORDS, dtype=t.uint8, device=eng.device)
    d_nodes = t.full(((allocated + GUARD_NODES) * 4,), SENTINEL, dtype=t.int32, device=eng.device)
    d_state = t.full((3 + GUARD_WORDS,), SENTINEL, dtype=t.int32, device=eng.device)
    d_cyc = t.full((3 + GUARD_WORDS,), SENTINEL, dtype=t.int64, device=eng.device)
    assert d_nodes.data_ptr() % 16 == 0
    _abi.check(eng.lib.kh_heap_flood(topl, profile, sx, sy, sz, float(c.an[0]), float(c.an[1]), float(c.an[2]), P(d_nbr),
                                     eng.optr(d_gate), P(d_dbf), P(d_alive), P(d_path), int(d_path.numel()), 1.0, 0.0, 0, sx - 1,
                                     P(d_nodes), allocated, capacity, P(d_state), P(d_cyc), eng.stream()))
    t.cuda.synchronize()
    state = d_state.cpu().numpy().view(np.uint32)
    cyc = d_cyc.cpu().numpy()
    alive = d_alive.cpu().numpy()
    nodes = d_nodes.cpu().numpy().view(np.uint32).reshape(-1, 4)
    assert np.all(state[3:] == SENTINEL) and np.all(cyc[3:] == SENTINEL) and np.all(alive[nvox:] == 1)
    # nothing outside [TOP, capacity) of the heap's memory was written (slot TOP is the clamp slot: read whatever the capacity is)
    assert np.all(nodes[:TOP[topl]] == SENTINEL), "a slot that lives in LDS was written in memory"
    assert np.all(nodes[max(capacity, TOP[topl] + 1):] == SENTINEL), "a slot at or behind the capacity was written"
    return int(state[0]), int(state[1]), int(state[2]), cyc[:3].copy(), alive[:nvox].reshape(c.shape, order="F"), nodes


@pytest.mark.parametrize("radii", sorted(FC.RADII))
@pytest.mark.parametrize("row", sorted(FC.ALL_ROWS))
def test_flood_alone_all_builds(eng, row, radii):
    """every row (the graph rows through kh_apply_voxel_graph and its corner gate), in its window, through the four builds"""
    c = FC.case(row, radii)
    print("%s/%s: oracle count %d, pushes %d, peak heap %d" % (row, radii, c.count, c.pushes, c.peak))
    assert FC.in_window(c), "the input left its regime: peak heap %d not in (%d, %d)" % ((c.peak,) + c.window)
    pushes = {}
    for topl, profile in BUILDS:
        what = "Heap<%d>%s" % (topl, ", profiled" if profile else "")
        cnt, pushes[topl, profile], status, cyc, after, nodes = run_flood(eng, c, topl, profile)
        print("  %s: count %d, pushes %d, status %d, cycles %s" % (what, cnt, pushes[topl, profile], status, cyc.tolist()))
        assert status == 0, what
        assert cnt == c.count, what
        np.testing.assert_array_equal(after, c.after, err_msg=what)
        if profile:
            assert np.all(cyc > 0), "%s: the cycle split of a flood that pops must be nonzero, got %s" % (what, cyc.tolist())
        else:
            assert np.all(cyc == 0), "%s: cycles without the profile, %s" % (what, cyc.tolist())
        if c.peak > TOP[topl] + 1:
            assert np.any(nodes[TOP[topl] + 1:c.peak] != SENTINEL), "%s: the heap never reached its memory" % what
    assert len(set(pushes.values())) == 1, "the builds disagree on the pushes: %s" % pushes
    assert pushes[1, 0] == c.pushes, "the oracle made %d pushes, the builds %d" % (c.pushes, pushes[1, 0])


@pytest.mark.parametrize("topl", [1, 2])
def test_flood_capacity_edge(eng, topl):
    """capacity == peak: every push fits, the oracle's result.  capacity == peak - 1: one push is refused, which is a status bit and
    nothing else -- the node buffer ends at the capacity and the 64 guard nodes behind it stay untouched in both runs."""
    c = FC.case("straddle", "differ")
    assert c.peak > TOP[2] + 1                         # so the buffer is exactly `capacity` nodes for both heaps
    cnt, pushes, status, _, after, nodes = run_flood(eng, c, topl, 0, capacity=c.peak)
    assert len(nodes) == c.peak + GUARD_NODES and np.all(nodes[c.peak:] == SENTINEL)
    assert status == 0 and cnt == c.count and pushes == c.pushes
    np.testing.assert_array_equal(after, c.after)
    assert np.any(nodes[c.peak - 1] != SENTINEL), "the last slot of the capacity was never used: the peak is not the peak"
    cnt, pushes, status, _, after, nodes = run_flood(eng, c, topl, 0, capacity=c.peak - 1)
    assert len(nodes) == c.peak - 1 + GUARD_NODES and np.all(nodes[c.peak - 1:] == SENTINEL)
    assert status & ST_HEAP_OVERFLOW, "a push beyond the capacity must set KH_ST_HEAP_OVERFLOW (status %d)" % status
    assert status == ST_HEAP_OVERFLOW


def test_flood_arguments_are_validated(eng):
    from kimimaro_amd import _abi
    t, P = eng.torch, eng.ptr
    c = FC.case("small", "equal")
    d_nbr, d_gate, d_dbf, d_path = device_inputs(eng, c)
    sx, sy, sz = c.shape
    d_alive = t.ones(sx * sy * sz, dtype=t.uint8, device=eng.device)
    buf = t.zeros(4 * 8300, dtype=t.int32, device=eng.device)
    st = t.zeros(3, dtype=t.int32, device=eng.device)
    cyc = t.zeros(3, dtype=t.int64, device=eng.device)

    def call(topl=1, profile=0, nodes=None, allocated=8300, capacity=4096, xmax=sx - 1):
        return eng.lib.kh_heap_flood(topl, profile, sx, sy, sz, 1.0, 1.0, 1.0, P(d_nbr), None, P(d_dbf), P(d_alive), P(d_path), 3,
                                     1.0, 0.0, 0, xmax, P(buf) if nodes is None else nodes, allocated, capacity, P(st), P(cyc),
                                     eng.stream())

    def refused(**kw):
        rc = call(**kw)
        assert rc == 1, "%s: expected KH_EINVAL, got %d" % (kw, rc)
        assert "kh_heap_flood" in _abi.last_error()

    refused(topl=0)
    refused(topl=3)
    refused(profile=2)
    refused(nodes=buf.data_ptr() + 4)                  # 16-byte alignment
    refused(nodes=0)
    refused(allocated=127)                              # TOP + 1 nodes for Heap<1>
    refused(topl=2, allocated=8191)                     # ... and for Heap<2>
    refused(allocated=4095)                             # below the capacity
    refused(xmax=sx)
    t.cuda.synchronize()
    assert st.cpu().tolist() == [0, 0, 0] and int(d_alive.sum().item()) == sx * sy * sz      # nothing ran
    _abi.check(call(topl=2, allocated=8192))
    t.cuda.synchronize()
    assert st.cpu().tolist()[0] == c.count and st.cpu().tolist()[2] == 0


# ---- the same heap inside the path kernel, and the knobs nobody sets ---------------------------------------------------------
def configure(name):
    """the engine of a variant: sweep off (every call is the heap emulation), two labels, the larger one on the second stream"""
    from kimimaro_amd.engine import Engine
    e = Engine()
    e.sweep = False
    e.split_min_voxels = 1
    e.split_slots = 1
    if name == "small_heap":
        e.big_lds_heap = False
    elif name == "profile_small_heap":
        e.profile = True
        e.big_lds_heap = False
    elif name == "profile_big_heap":
        e.profile = True
    elif name == "heap_prio":
        e.heap_prio = True
    elif name == "big_threads_64":
        e.big_threads = 64
    elif name == "big_threads_128":
        e.big_threads = 128
    elif name == "lanes_big_heap":
        e.trace_threads = 64
        e.big_lds_labels = 1
    elif name == "lanes_small_heap":
        e.trace_threads = 64
    else:
        assert name == "default"
    assert e.big_lds_heap == (name not in ("small_heap", "profile_small_heap")) and (e.big_lds_labels is None) == (name != "lanes_big_heap")
    return e


_runs = {}


def path_run(name):
    """skeletons, final task records and the (big, flag word) of every launch of the variant; once per module"""
    if name not in _runs:
        import kimimaro_amd
        pc = FC.path_case()
        e = configure(name)
        launches = []
        flags_of = e.trace_flags

        def recorded(*args, **kwargs):
            word = flags_of(*args, **kwargs)
            launches.append((bool(kwargs.get("big", False)), word))
            return word

        e.trace_flags = recorded
        got = kimimaro_amd.skeletonize(FC.path_volume(), pc.params, anisotropy=pc.an, dust_threshold=0, fix_borders=False,
                                       progress=False, _engine=e)
        _runs[name] = (got, e.last_tasks.copy(), launches)
    return _runs[name]


def check_path_run(name):
    """the oracle's skeletons, no sweep, one big and one small launch; -> (record of the block, record of the bar, flag word of the big
    launch, of the small one)"""
    pc = FC.path_case()
    got, tk, launches = path_run(name)
    print("%s: launches %s, pushes %s, kcyc pop/push/fire %s" % (name, [(b, hex(w)) for b, w in launches], tk["stat_heap_pushes"].tolist(),
                                                               [tk[k].tolist() for k in ("cyc_pop", "cyc_push", "cyc_fire")]))
    assert sorted(got.keys()) == sorted(pc.want.keys()) == [1, 2]
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, pc.want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, pc.want[k].edges)
        np.testing.assert_allclose(got[k].radii, pc.want[k].radii, rtol=1e-4)
    assert len(tk) == 2 and int(tk["stat_sweep_calls"].sum()) == 0 and not tk["status"].any()
    block, bar = tk[np.argmax(tk["count"])], tk[np.argmin(tk["count"])]
    assert int(block["count"]) == int(np.prod(FC.BLOCK)) and int(bar["count"]) == 24
    # the pushes of all floods of a label are the oracle's (the oracle floods each label on its own crop)
    want_block = sum(c[3] for c in pc.calls if c[0] == FC.BLOCK)
    want_bar = sum(c[3] for c in pc.calls if c[0] != FC.BLOCK)
    assert want_block > FC.PARENTS_HBM[0] and want_bar > 0
    assert (int(block["stat_heap_pushes"]), int(bar["stat_heap_pushes"])) == (want_block, want_bar)
    assert [b for b, _ in launches] == [True, False], "one launch of the largest label on the second stream, one of the rest"
    return block, bar, launches[0][1], launches[1][1]


CYCLES = ("cyc_pop", "cyc_push", "cyc_fire")


def test_path_default_engine_runs_the_big_lds_heap():
    """the default engine: the block's launch carries KH_TRACE_BIG_LDS_HEAP (Heap<2> inside trace_paths_kernel<false, 2>, its flood
    peaking at 16 976 nodes) and makes the pushes the Heap<1> engine makes; nothing is profiled"""
    from kimimaro_amd import _abi as A
    block, bar, big, small = check_path_run("default")
    assert big & A.TRACE_BIG_LDS_HEAP and not small & A.TRACE_BIG_LDS_HEAP
    assert not (big | small) & (A.TRACE_PROFILE | A.TRACE_HEAP_PRIO | A.TRACE_THREADS_64 | A.TRACE_THREADS_128)
    block1, bar1, big1, small1 = check_path_run("small_heap")
    assert not (big1 | small1) & A.TRACE_BIG_LDS_HEAP
    assert int(block["stat_heap_pushes"]) == int(block1["stat_heap_pushes"])
    assert int(bar["stat_heap_pushes"]) == int(bar1["stat_heap_pushes"])
    for rec in (block, bar, block1, bar1):
        assert [int(rec[k]) for k in CYCLES] == [0, 0, 0]


def test_path_profiled_build():
    """profile = True without the big heap: both launches carry KH_TRACE_PROFILE (trace_paths_kernel<true, 1>) and both labels,
    which push, get a nonzero pop / push / fire cycle split"""
    from kimimaro_amd import _abi as A
    block, bar, big, small = check_path_run("profile_small_heap")
    assert big & A.TRACE_PROFILE and small & A.TRACE_PROFILE and not (big | small) & A.TRACE_BIG_LDS_HEAP
    for rec in (block, bar):
        assert all(int(rec[k]) > 0 for k in CYCLES), [int(rec[k]) for k in CYCLES]
    block0 = check_path_run("small_heap")[0]
    assert int(block["stat_heap_pushes"]) == int(block0["stat_heap_pushes"])


def test_path_profile_with_big_heap_runs_unprofiled():
    """profile = True with the big heap on: the engine sets KH_TRACE_PROFILE and KH_TRACE_BIG_LDS_HEAP on the block's launch, and
    kh_trace_paths looks at KH_TRACE_BIG_LDS_HEAP first (there is no profiled trace_paths_kernel<., 2>): that launch runs
    UNPROFILED -- its label's cycle split stays zero while the bar's, from the profiled Heap<1> launch, is filled.  Known and left
    as it is; a profile of the largest labels needs big_lds_heap = False."""
    from kimimaro_amd import _abi as A
    block, bar, big, small = check_path_run("profile_big_heap")
    assert big & A.TRACE_PROFILE and big & A.TRACE_BIG_LDS_HEAP, "both flags reach kh_trace_paths on the big launch"
    assert small & A.TRACE_PROFILE and not small & A.TRACE_BIG_LDS_HEAP
    assert [int(block[k]) for k in CYCLES] == [0, 0, 0]
    assert all(int(bar[k]) > 0 for k in CYCLES)
    assert int(block["stat_heap_pushes"]) == int(check_path_run("default")[0]["stat_heap_pushes"])


def test_path_heap_prio():
    from kimimaro_amd import _abi as A
    block, bar, big, small = check_path_run("heap_prio")
    assert big & A.TRACE_HEAP_PRIO and small & A.TRACE_HEAP_PRIO and big & A.TRACE_BIG_LDS_HEAP
    assert int(block["stat_heap_pushes"]) == int(check_path_run("default")[0]["stat_heap_pushes"])


@pytest.mark.parametrize("threads", [64, 128])
def test_path_big_threads(threads):
    """the big launch with a thread count of its own: Heap<2> with one and with two waves per label, the rest with 256 threads"""
    from kimimaro_amd import _abi as A
    block, bar, big, small = check_path_run("big_threads_%d" % threads)
    mine, other = (A.TRACE_THREADS_64, A.TRACE_THREADS_128) if threads == 64 else (A.TRACE_THREADS_128, A.TRACE_THREADS_64)
    assert big & mine and not big & other and big & A.TRACE_BIG_LDS_HEAP
    assert not small & (A.TRACE_THREADS_64 | A.TRACE_THREADS_128 | A.TRACE_BIG_LDS_HEAP)
    assert int(block["stat_heap_pushes"]) == int(check_path_run("default")[0]["stat_heap_pushes"])


def test_path_lanes_form_of_the_big_launch():
    """trace_threads = 64: with big_lds_labels = 1 the block's launch is the lanes' form of the big launch -- KH_TRACE_BIG_LDS_HEAP
    together with KH_TRACE_THREADS_64; with big_lds_labels unset one wave per label means Heap<1>, the flag must be absent"""
    from kimimaro_amd import _abi as A
    block, bar, big, small = check_path_run("lanes_big_heap")
    assert big & A.TRACE_BIG_LDS_HEAP and big & A.TRACE_THREADS_64
    assert small & A.TRACE_THREADS_64 and not small & A.TRACE_BIG_LDS_HEAP
    block1, bar1, big1, small1 = check_path_run("lanes_small_heap")
    assert not (big1 | small1) & A.TRACE_BIG_LDS_HEAP and big1 & A.TRACE_THREADS_64 and small1 & A.TRACE_THREADS_64
    assert int(block["stat_heap_pushes"]) == int(block1["stat_heap_pushes"]) == int(check_path_run("default")[0]["stat_heap_pushes"])
