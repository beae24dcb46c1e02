"""The scripts tests/test_gpu_heap_script.py runs through kh_heap_script and tests/test_heap_ref_host.py through std::priority_queue:
one case = one launch.  A case carries the regime of csrc/heap.h it is built for (`regime`: peak = the peak size lies strictly
between the two; reach = (slot B, count): more than `count` pops walked their hole to a slot >= B; cross = B: pops on both sides of
size B and a node moved across the slot pair; refused = pushes a capacity drops); the host test asserts, on the reference alone,
that the case is in it.

Shapes (the smallest that reach each path): drain_small -- N = 1..200: push N, dump, pop all; boundary -- grow to B + 70, then four
times pop 140 / push 140 with a dump at the sizes B-1 .. B+2 both ways; mirror_deep -- 6 000 nodes, 3 000 pop/push pairs;
one_chunk -- 40 000 nodes and 5 000 mixed operations; two_chunks -- grow past B = 131 071 (Heap<1>) or 524 287 (Heap<2>), a saw
tooth of +-200 across B three times, then a tail of pops and one full dump; capacity -- capacity + 50 pushes, 30 pops, 60 pushes,
pop all.

Key families (each a function of a seeded np.random.default_rng; keys are float32 bit patterns, all below +inf):
  equal        one value: with `>=` every push climbs to the root
  ascending    distinct, rising: no push climbs          descending   distinct, falling by 1..3 ulp: every push climbs to the root
  few          {0.0, 1.0, nextafter(1, 2), 2.0}
  bits         random non-negative finite patterns: normals, denormals, 0.0, and values that differ only in their low two bits
  flood        pop the minimum, then push keys >= the popped key from a table of sqrt(a^2 + b^2 + c^2): many exact ties
Payloads are unique per push (a running number), so a wrong tie order cannot hide behind equal records."""
import functools
import heapq
import zlib

import numpy as np

import heap_ref as HR

TOP = HR.TOP
FAMILIES = ("equal", "ascending", "descending", "few", "bits", "flood")


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def flood_table(r=48):
    """the flood's keys of the offsets (a, b, c), float operation order of the kernel (s = a*a; s += b*b; s += c*c; sqrt)"""
    a = np.arange(r, dtype=np.float32)
    s = (a * a)[:, None, None] + (a * a)[None, :, None]
    s = s + (a * a)[None, None, :]
    return np.unique(np.sqrt(s.astype(np.float32)).astype(np.float32))


FLOOD_TABLE = flood_table()
FEW = [f32_bits(0.0), f32_bits(1.0), f32_bits(np.nextafter(np.float32(1), np.float32(2))), f32_bits(2.0)]


class Keys:
    """k keys of a family; `floor` (bits) is the key popped last -- only the flood looks at it"""

    def __init__(self, family, rng):
        assert family in FAMILIES
        self.family, self.rng = family, rng
        self.cur = 0x3F800000 if family == "ascending" else 0x4B000000

    def take(self, k, floor):
        rng, fam = self.rng, self.family
        if fam == "equal":
            return [0x40490FDB] * k
        if fam == "few":
            return [FEW[i] for i in rng.integers(0, 4, k)]
        if fam in ("ascending", "descending"):
            steps = np.cumsum(rng.integers(1, 4, k))
            out = self.cur + steps if fam == "ascending" else self.cur - steps
            if k:
                self.cur = int(out[-1])
            return [int(v) for v in out]
        if fam == "bits":
            kind = rng.choice(4, size=k, p=[0.5, 0.2, 0.25, 0.05])
            cols = [rng.integers(0x00800000, 0x7F800000, k), rng.integers(1, 0x00800000, k), 0x3F800000 + rng.integers(0, 4, k),
                    np.zeros(k, dtype=np.int64)]
            return [int(cols[kd][i]) for i, kd in enumerate(kind)]
        i0 = int(np.searchsorted(FLOOD_TABLE, np.uint32(floor).view(np.float32), side="left"))
        idx = np.minimum(i0 + rng.integers(0, 30, k), len(FLOOD_TABLE) - 1)
        return [int(v) for v in FLOOD_TABLE[idx].view(np.uint32)]


class Builder:
    """writes the records and keeps the multiset of keys (the popped key is the minimum whatever the tie order is)"""

    def __init__(self, family, seed, capacity=None):
        self.rng = np.random.default_rng(seed)
        self.keys = Keys(family, self.rng)
        self.flood = family == "flood"
        self.recs, self.heap = [], []
        self.capacity = capacity
        self.payload = 0
        self.floor = 0

    @property
    def n(self):
        return len(self.heap)

    def push(self, k=1):
        for key in self.keys.take(k, self.floor):
            assert 0 <= key < 0x7F800000
            self.recs.append((HR.OP_PUSH, key, self.payload, int(self.rng.integers(0, 8))))
            self.payload += 1
            if self.capacity is None or self.n < self.capacity:
                heapq.heappush(self.heap, key)

    def pop(self, k=1):
        for _ in range(k):
            self.floor = heapq.heappop(self.heap)
            self.recs.append((HR.OP_POP, 0, 0, 0))

    def dump(self, size_only=False):
        self.recs.append((HR.OP_DUMP, HR.DUMP_SIZE_ONLY if size_only else 0, 0, 0))

    def grow(self, target):
        """to `target` nodes: plain pushes, or -- the flood -- pop one, push 0..26, as the flood's front does"""
        if self.flood:
            if self.n == 0:
                self.push()
            while self.n < target - 26:
                self.pop()
                self.push(int(self.rng.integers(0, 27)) or (1 if self.n == 0 else 0))
        self.push(target - self.n)
        assert self.n == target

    def mixed(self, count):
        """`count` operations that keep the size about where it is"""
        done = 0
        while done < count:
            if self.flood:
                k = int(self.rng.integers(0, 3))
                self.pop()
                self.push(k)
                done += 1 + k
            else:
                if self.rng.integers(0, 2) and self.n:
                    self.pop()
                else:
                    self.push()
                done += 1

    def ops(self):
        return np.array(self.recs, dtype=np.uint32).reshape(-1, 4)


def seed_of(name):
    return zlib.crc32(name.encode())


# ---- the shapes -------------------------------------------------------------------------------------------------------------
def drain_small(b):
    for n in range(1, 201):
        b.push(n)
        b.dump()
        b.pop(n)


def boundary(b, B):
    b.grow(B + 70)
    b.dump()
    marks = (B - 1, B, B + 1, B + 2)
    for _ in range(4):
        for _ in range(140):
            b.pop()
            if b.n in marks:
                b.dump()
        for _ in range(140):
            b.push()
            if b.n in marks:
                b.dump()


def mirror_deep(b):
    b.grow(6000)
    for i in range(3000):
        b.pop()
        b.push()
        if (i + 1) % 500 == 0:
            b.dump()


def one_chunk(b):
    b.grow(40000)
    for _ in range(3):
        b.mixed(1250)
        b.dump()
    b.mixed(1250)
    b.dump()


def two_chunks(b, B=131071, peak=150000, tail=20000):
    b.grow(peak)
    b.dump(size_only=True)
    for _ in range(3):
        b.pop(b.n - (B - 200))
        b.dump(size_only=True)
        b.push(B + 200 - b.n)
        b.dump(size_only=True)
    b.pop(tail)
    b.dump()


def capacity_shape(b):
    cap = b.capacity
    b.push(cap + 50)
    b.dump()
    b.pop(30)
    b.push(60)
    b.dump()
    b.pop(b.n)


def _case(name, topl, family, shape, regime, capacity=None, big=False):
    return dict(name=name, topl=topl, family=family, shape=shape, regime=regime, capacity=capacity, big=big)


def _all_cases():
    out = []
    for topl in (1, 2):
        for fam in ("equal", "few", "bits", "descending", "ascending"):
            out.append(_case("drain_small-%d-%s" % (topl, fam), topl, fam, drain_small, dict(peak=(199, 201))))
    for topl, B in ((1, 127), (1, 2047), (2, 127), (2, 8191)):
        for fam in ("few", "flood", "equal"):
            out.append(_case("boundary-%d-%d-%s" % (topl, B, fam), topl, fam, functools.partial(boundary, B=B), dict(cross=B)))
    out.append(_case("mirror_deep-1-flood", 1, "flood", mirror_deep, dict(peak=(2047, 8191), reach=(2047, 1000))))
    for topl in (1, 2):
        for fam in ("few", "flood"):
            regime = dict(peak=(2047, 131071)) if topl == 1 else dict(peak=(8191, 524287), reach=(8191, 1000))
            out.append(_case("one_chunk-%d-%s" % (topl, fam), topl, fam, one_chunk, regime))
    for fam in ("flood", "few"):
        out.append(_case("two_chunks-1-%s" % fam, 1, fam, two_chunks, dict(peak=(131071, 1 << 20), reach=(131071, 1000), cross=131071),
                         big=True))
    # Heap<2>'s second global chunk: the same shape across 524 287, a shorter tail
    out.append(_case("two_chunks-2-few", 2, "few", functools.partial(two_chunks, B=524287, peak=530000, tail=4000),
                     dict(peak=(524287, 1 << 22), reach=(524287, 1000), cross=524287), big=True))
    for topl, caps in ((1, (64, 100, 126, 127, 128, 2047, 2048)), (2, (8191, 8192))):
        for cap in caps:
            for fam in ("few", "bits"):
                out.append(_case("capacity-%d-%d-%s" % (topl, cap, fam), topl, fam, capacity_shape, dict(refused=50 + 30), capacity=cap))
    return out


CASES = _all_cases()
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
assert len(BY_NAME) == len(CASES)


class Built:
    pass


@functools.lru_cache(maxsize=None)
def built(name):
    """the case's script (read-only), its capacity and buffer sizes, and the reference's result -- made once, shared"""
    case = BY_NAME[name]
    b = Builder(case["family"], seed_of(name), capacity=case["capacity"])
    case["shape"](b)
    out = Built()
    out.case = case
    out.topl = case["topl"]
    out.ops = b.ops()
    out.ops.setflags(write=False)
    peak_needed = max(200, int((out.ops[:, 0] == HR.OP_PUSH).sum()))
    out.capacity = case["capacity"] if case["capacity"] is not None else peak_needed + 100
    out.nodes_allocated = max(out.capacity, TOP[out.topl] + 1)
    out.ref = HR.run(out.ops, out.capacity)
    return out
