"""tests/heap_ref.py (bits/stl_heap.h restated from the rule) against the std::priority_queue of the libstdc++ that is installed
(tests/heap_std.cpp, built here with g++ -O2), on every script of tests/heap_cases.py, without a GPU.  The GPU test compares
kh_heap_script with heap_ref; this file is what makes heap_ref a witness of "the array layout is libstdc++'s".

Also here, on the reference alone: every case is in the regime it is named for."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import heap_cases as HC
import heap_ref as HR

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def heap_std(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("heap_std") / "heap_std")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "heap_std.cpp")])
    return exe


def run_std(exe, ops, tmp_path):
    """(pops [npops, 4], dump words without mirror words) of the program on `ops`"""
    script, pops, dumps = (str(tmp_path / n) for n in ("script.bin", "pops.bin", "dumps.bin"))
    np.ascontiguousarray(ops, dtype=np.uint32).tofile(script)
    subprocess.check_call([exe, script, pops, dumps])
    return np.fromfile(pops, dtype=np.uint32).reshape(-1, 4), np.fromfile(dumps, dtype=np.uint32)


def plain_dump_words(res, only_last=False):
    """the reference's dumps in the program's form: header, nodes, no mirror words"""
    out = []
    for n, at, nodes in (res.dumps[-1:] if only_last else res.dumps):
        out.append(np.array([n, at], dtype=np.uint32))
        if nodes is not None:
            out.append(nodes.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def without_refused(ops, capacity):
    """the script with the pushes a capacity refuses taken out: only sizes are counted here, no heap is kept.  Dump headers carry
    their record's index, so the index map comes back too."""
    keep, n = [], 0
    for i, (op, _, _, _) in enumerate(ops.tolist()):
        if op == HR.OP_PUSH:
            if n >= capacity:
                continue
            n += 1
        elif op == HR.OP_POP:
            n -= 1
        keep.append(i)
    return ops[keep], np.array(keep)


@pytest.mark.parametrize("name", HC.NAMES)
def test_reference_equals_libstdcxx(heap_std, tmp_path, name):
    b = HC.built(name)
    ref = b.ref
    assert ref.errors == 0
    if b.case["capacity"] is None:
        assert ref.refused == 0
        ops, index = b.ops, None
    else:
        # the reference drops a refused push; std::priority_queue gets the script without those pushes
        ops, index = without_refused(b.ops, b.capacity)
        assert len(b.ops) - len(ops) == ref.refused > 0
    pops, dumps = run_std(heap_std, ops, tmp_path)
    np.testing.assert_array_equal(ref.pops, pops)
    want = plain_dump_words(ref)
    if index is not None:
        # dump headers: the program saw the shortened script's indices
        pos = 0
        dumps = dumps.copy()
        for n, at, nodes in ref.dumps:
            dumps[pos + 1] = index[dumps[pos + 1]]
            pos += 2 + (0 if nodes is None else 4 * n)
        assert pos == len(dumps)
    if b.case["big"]:
        # the largest (two_chunks: their other dumps are of the size only): pops and the final dump
        last = plain_dump_words(ref, only_last=True)
        np.testing.assert_array_equal(dumps[len(dumps) - len(last):], last)
    else:
        np.testing.assert_array_equal(dumps, want)


@pytest.mark.parametrize("name", HC.NAMES)
def test_case_is_in_its_regime(name):
    """asserted on the reference alone: what the case is named for happens in it"""
    b = HC.built(name)
    ref, regime, fam = b.ref, b.case["regime"], b.case["family"]
    print(name, "ops", len(b.ops), "pops", len(ref.pops), "dumps", len(ref.dumps), "peak", ref.peak, "climbs", ref.climbs,
          "reach", ref.reach, "land", ref.land)
    assert ref.errors == 0
    payloads = b.ops[b.ops[:, 0] == HR.OP_PUSH, 2]
    assert len(np.unique(payloads)) == len(payloads)
    assert int(b.ops[b.ops[:, 0] == HR.OP_PUSH, 1].max()) < 0x7F800000
    if "peak" in regime:
        lo, hi = regime["peak"]
        assert lo < ref.peak < hi
    if "reach" in regime:
        B, count = regime["reach"]
        assert ref.reach[B] > count, "too few pops whose path went below slot %d" % B
    if "cross" in regime:
        B = regime["cross"]
        assert ref.lens_below[B] > 0 and ref.lens_above[B] > 0, "pops on one side of %d only" % B
        assert ref.reach[B] > 0
        # With one key value nothing is smaller than the former last element: libstdc++ walks the hole down across the pair and
        # pushes the element all the way up again, the net move across the pair is none.  Every other family must move a node.
        assert (ref.land[B] == 0) if fam == "equal" else (ref.land[B] > 0)
    if "refused" in regime:
        assert ref.refused == regime["refused"]
        assert ref.peak == b.capacity
    if fam in ("equal", "descending"):
        # with `>=` a key that is no larger than every key in the heap climbs to the root: every accepted push but those into
        # an empty heap leaves its leaf
        n, into_nonempty = 0, 0
        for op in b.ops[:, 0].tolist():
            if op == HR.OP_PUSH and n < b.capacity:
                into_nonempty += n > 0
                n += 1
            elif op == HR.OP_POP:
                n -= 1
        assert ref.climbs == into_nonempty > 0
    if fam == "ascending":
        assert ref.climbs == 0
    if name.startswith("drain_small"):
        # every size 1..200 was drained one pop at a time: every single-child hole (len == 2 * nh + 2) of the LDS part occurred
        sizes = set(ref.pops[:, 3].tolist())
        assert sizes == set(range(1, 201))
