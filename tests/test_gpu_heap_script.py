"""The invalidation heap of csrc/heap.h on its own: kh_heap_script runs a script of pushes, pops and dumps on Heap<1> (127 slots in
LDS, the key mirror of slots 127..2046) and Heap<2> (8 191 slots in LDS) exactly as the path loop builds them, and every word it
returns is compared with tests/heap_ref.py -- libstdc++'s __push_heap / __adjust_heap restated, which tests/test_heap_ref_host.py
has pinned to the installed std::priority_queue and which says, per case, that the case is in the regime it is named for.

Exact comparisons (uint32 words): every pop record {key, payload, source, n before}, every dump (all nodes in slot order: "the
array layout after every operation is identical to libstdc++'s"), the mirror words against the REFERENCE's keys of those slots,
and the state words.  The node buffer is filled with a sentinel and has 64 guard nodes behind it: slots below TOP (they live in
LDS) and slots from max(capacity, TOP + 1) on must come back untouched.

The batched append of invalidate_ball is not reached from here (it is part of the flood's loop): tests/test_gpu_heap_flood.py
(kh_heap_flood, both heaps, at the sizes where the append's selects switch), tests/test_gpu_heap_mirror.py and
tests/test_gpu_trace.py cover it through whole floods."""
import time

import numpy as np
import pytest

import heap_cases as HC
import heap_ref as HR

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD_NODES = 64
GUARD_WORDS = 64


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def run_script(eng, topl, ops, capacity, nodes_allocated, pops_words, dumps_words):
    """one launch: (pops buffer, dumps buffer, state, node buffer [nodes_allocated + GUARD_NODES, 4], seconds)"""
    from kimimaro_amd import _abi
    t, P = eng.torch, eng.ptr
    dev = eng.device
    d_ops = t.from_numpy(np.ascontiguousarray(ops).view(np.int32).reshape(-1).copy()).to(dev)
    d_nodes = t.full(((nodes_allocated + GUARD_NODES) * 4,), SENTINEL, dtype=t.int32, device=dev)
    d_pops = t.full((pops_words + GUARD_WORDS,), SENTINEL, dtype=t.int32, device=dev)
    d_dumps = t.full((dumps_words + GUARD_WORDS,), SENTINEL, dtype=t.int32, device=dev)
    d_state = t.full((4 + GUARD_WORDS,), SENTINEL, dtype=t.int32, device=dev)
    assert d_nodes.data_ptr() % 16 == 0
    t.cuda.synchronize()
    t0 = time.perf_counter()
    _abi.check(eng.lib.kh_heap_script(topl, P(d_ops), len(ops), P(d_nodes), nodes_allocated, capacity, P(d_pops), pops_words,
                                      P(d_dumps), dumps_words, P(d_state), eng.stream()))
    t.cuda.synchronize()
    dt = time.perf_counter() - t0
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    return u32(d_pops), u32(d_dumps), u32(d_state), u32(d_nodes).reshape(-1, 4), dt


@pytest.mark.parametrize("name", HC.NAMES)
def test_heap_script(eng, name):
    b = HC.built(name)
    ref, topl = b.ref, b.topl
    want_pops = ref.pops.reshape(-1)
    want_dumps = ref.dump_words(topl)
    pops, dumps, state, nodes, dt = run_script(eng, topl, b.ops, b.capacity, b.nodes_allocated, len(want_pops), len(want_dumps))
    print("%s: %d records, %d pops, %d dump words, peak %d, kernel %.3f s" % (name, len(b.ops), len(ref.pops), len(want_dumps),
                                                                            ref.peak, dt))
    np.testing.assert_array_equal(state[:4], [ref.n, ref.refused, 0, 0])
    np.testing.assert_array_equal(pops[:len(want_pops)], want_pops)
    # dump by dump, so that a failure names the dump, the slot and whether it is a node or a mirror word
    pos = 0
    for n, at, want_nodes in ref.dumps:
        np.testing.assert_array_equal(dumps[pos:pos + 2], [n, at], err_msg="header of the dump at record %d" % at)
        pos += 2
        if want_nodes is None:
            continue
        got_nodes = dumps[pos:pos + 4 * n].reshape(n, 4)
        np.testing.assert_array_equal(got_nodes, want_nodes, err_msg="nodes of the dump at record %d (n = %d)" % (at, n))
        pos += 4 * n
        nmir = max(0, min(n, HR.MIR_END[topl]) - HR.TOP[topl])
        np.testing.assert_array_equal(dumps[pos:pos + nmir], want_nodes[HR.TOP[topl]:HR.TOP[topl] + nmir, 0],
                                      err_msg="mirror words of the dump at record %d (n = %d)" % (at, n))
        pos += nmir
    assert pos == len(want_dumps)
    np.testing.assert_array_equal(dumps, np.concatenate([want_dumps, np.full(GUARD_WORDS, SENTINEL, np.uint32)]))
    assert np.all(pops[len(want_pops):] == SENTINEL) and np.all(state[4:] == SENTINEL)
    # nothing outside [TOP, capacity) of the slice was written (slot TOP itself is the clamp slot: read whatever the capacity is)
    top = HR.TOP[topl]
    assert np.all(nodes[:top] == SENTINEL), "a slot that lives in LDS was written in memory"
    assert np.all(nodes[max(b.capacity, top + 1):] == SENTINEL), "a slot at or behind the capacity was written"
    if b.capacity <= top:
        assert np.all(nodes == SENTINEL)


def test_output_capacities_and_script_errors(eng):
    """pop records and dumps that do not fit are dropped whole and counted, the heap goes on; a pop of an empty heap and a record
    that is no op are counted and skipped"""
    key = HC.f32_bits(1.0)
    ops = np.array([(HR.OP_POP, 0, 0, 0), (HR.OP_PUSH, key, 1, 0), (HR.OP_PUSH, key, 2, 0), (HR.OP_PUSH, key, 3, 0), (7, 0, 0, 0),
                    (HR.OP_DUMP, 0, 0, 0), (HR.OP_POP, 0, 0, 0), (HR.OP_POP, 0, 0, 0), (HR.OP_DUMP, HR.DUMP_SIZE_ONLY, 0, 0),
                    (HR.OP_POP, 0, 0, 0), (HR.OP_POP, 0, 0, 0)], dtype=np.uint32)
    ref = HR.run(ops, 100)
    assert ref.errors == 3 and len(ref.pops) == 3
    for topl in (1, 2):
        pops, dumps, state, nodes, _ = run_script(eng, topl, ops, 100, HR.TOP[topl] + 1, 7, 3)
        np.testing.assert_array_equal(state[:4], [0, 0, 3, 3])                 # the dump of 14 words, two of three pop records
        np.testing.assert_array_equal(pops[:4], ref.pops[0])
        assert np.all(pops[4:] == SENTINEL)
        np.testing.assert_array_equal(dumps[:2], [1, 8])
        assert np.all(dumps[2:] == SENTINEL) and np.all(nodes == SENTINEL)


def test_arguments_are_validated(eng):
    from kimimaro_amd import _abi
    t, P = eng.torch, eng.ptr
    buf = t.zeros(4 * 256, dtype=t.int32, device=eng.device)
    st = t.zeros(4, dtype=t.int32, device=eng.device)
    L = eng.lib
    assert L.kh_heap_script(3, None, 0, P(buf), 256, 10, None, 0, None, 0, P(st), eng.stream()) != 0          # topl
    assert L.kh_heap_script(1, None, 0, P(buf), 127, 10, None, 0, None, 0, P(st), eng.stream()) != 0          # TOP + 1 nodes
    assert L.kh_heap_script(1, None, 0, P(buf), 256, 257, None, 0, None, 0, P(st), eng.stream()) != 0         # capacity
    assert L.kh_heap_script(1, None, 0, buf.data_ptr() + 4, 128, 10, None, 0, None, 0, P(st), eng.stream()) != 0   # alignment
    assert L.kh_heap_script(1, None, 0, P(buf), 256, 10, None, -1, None, 0, P(st), eng.stream()) != 0
    assert L.kh_heap_script(2, None, 0, P(buf), 256, 10, None, 0, None, 0, P(st), eng.stream()) != 0          # 8 192 for Heap<2>
    _abi.check(L.kh_heap_script(1, None, 0, P(buf), 256, 10, None, 0, None, 0, P(st), eng.stream()))
    t.cuda.synchronize()
    assert st.cpu().tolist() == [0, 0, 0, 0]
