"""libstdc++'s std::priority_queue restated from bits/stl_heap.h -- __push_heap, __adjust_heap, __pop_heap -- with the flood's
comparator comp(a, b) = a.key >= b.key, on a Python list of (key bits, payload, source).  This is the rule, not csrc/heap.h:
no chunks, no lanes, no mirror.  tests/test_heap_ref_host.py pins it to the installed libstdc++ (tests/heap_std.cpp).

Keys are the bit patterns of non-negative finite floats: their order as unsigned integers is their order as floats.

The script format is kh_heap_script's (include/kimi_hip.h): records of four uint32 words."""
import numpy as np

OP_PUSH, OP_POP, OP_DUMP = 0, 1, 2
DUMP_SIZE_ONLY = 1
TOP = {1: 127, 2: 8191}                 # heap slots in LDS
MIR_END = {1: 2047, 2: 8191}            # slots TOP .. MIR_END-1 have their key in the LDS mirror (Heap<2> has none)
BOUNDARIES = (127, 2047, 8191, 131071, 524287)


def comp(a, b):
    return a[0] >= b[0]


def push_heap_(first, hole, top, value):
    """__push_heap: the value climbs from `hole` over every ancestor that compares true against it"""
    parent = (hole - 1) // 2
    while hole > top and comp(first[parent], value):
        first[hole] = first[parent]
        hole = parent
        parent = (hole - 1) // 2
    first[hole] = value
    return hole


def adjust_heap_(first, hole, length, value):
    """__adjust_heap: the hole walks to a leaf along the child that does not compare true against its sibling, then the value
    is pushed up from there.  Returns (the leaf the hole reached, the slot the value landed in)."""
    top = hole
    child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if comp(first[child], first[child - 1]):
            child -= 1
        first[hole] = first[child]
        hole = child
    if (length & 1) == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        first[hole] = first[child - 1]
        hole = child - 1
    return hole, push_heap_(first, hole, top, value)


class Queue:
    """std::priority_queue<Node, std::vector<Node>, Compare>: `c` is the protected container"""

    def __init__(self):
        self.c = []

    def push(self, node):
        self.c.append(node)
        return push_heap_(self.c, len(self.c) - 1, 0, node)

    def pop(self):
        """std::pop_heap + pop_back.  Returns (deepest slot the hole reached, slot the former last element landed in)."""
        c = self.c
        leaf = land = 0
        if len(c) > 1:
            value = c[-1]
            c[-1] = c[0]
            leaf, land = adjust_heap_(c, 0, len(c) - 1, value)
        c.pop()
        return leaf, land


class Result:
    """pops: uint32 [npops, 4] = {key, payload, source, n before the pop}; dumps: list of (n, op index, uint32 [n, 4] nodes or
    None for a dump of the size only); n: final size; refused: pushes dropped at n >= capacity; errors: pops of an empty heap and
    records that are no op.  Regime counters: peak; pop_lens (min, max of the size after a pop); for each boundary slot B of
    BOUNDARIES reach[B] = pops whose hole walked to a slot >= B, land[B] = pops after which the former last element sits at a
    slot >= B (so a node moved from a slot >= B to its parent below B), climbs = pushes that left their leaf."""

    def dump_words(self, topl):
        """the dumps as kh_heap_script writes them: {n, op index}, the nodes, the mirror words (the reference's keys)"""
        out = []
        for n, at, nodes in self.dumps:
            out.append(np.array([n, at], dtype=np.uint32))
            if nodes is not None:
                out.append(nodes.reshape(-1))
                out.append(nodes[TOP[topl]:min(n, MIR_END[topl]), 0])
        return np.concatenate(out) if out else np.zeros(0, np.uint32)


def run(ops, capacity):
    recs = np.asarray(ops, dtype=np.uint32).reshape(-1, 4).tolist()
    q = Queue()
    c = q.c
    res = Result()
    pops, dumps = [], []
    refused = errors = climbs = peak = 0
    lens_below = {b: 0 for b in BOUNDARIES}
    lens_above = {b: 0 for b in BOUNDARIES}
    reach = {b: 0 for b in BOUNDARIES}
    land = {b: 0 for b in BOUNDARIES}

    def push(node):
        nonlocal refused, climbs, peak
        if len(c) >= capacity:
            refused += 1                     # a refused push is simply dropped
            return
        leaf = len(c)
        if q.push(node) != leaf:
            climbs += 1
        if len(c) > peak:
            peak = len(c)

    i, nops = 0, len(recs)
    while i < nops:
        op, a, b, d = recs[i]
        if op == OP_PUSH:
            push((a, b, d))
        elif op == OP_POP:
            if not c:
                errors += 1
            else:
                k, p, s = c[0]
                pops.append((k, p, s, len(c)))
                leaf, where = q.pop()
                length = len(c)
                for bd in BOUNDARIES:
                    if length < bd:
                        lens_below[bd] += 1
                    else:
                        lens_above[bd] += 1
                    if leaf >= bd:
                        reach[bd] += 1
                    if where >= bd:
                        land[bd] += 1
        elif op == OP_DUMP:
            nodes = None
            if not (a & DUMP_SIZE_ONLY):
                nodes = np.zeros((len(c), 4), dtype=np.uint32)
                if c:
                    nodes[:, :3] = np.array(c, dtype=np.uint32)
            dumps.append((len(c), i, nodes))
        else:
            errors += 1
        i += 1
    res.pops = np.array(pops, dtype=np.uint32).reshape(-1, 4)
    res.dumps = dumps
    res.n = len(c)
    res.refused = refused
    res.errors = errors
    res.peak = peak
    res.climbs = climbs
    res.lens_below, res.lens_above, res.reach, res.land = lens_below, lens_above, reach, land
    return res
