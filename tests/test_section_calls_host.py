"""What tests/test_gpu_section_calls.py rests on, without a GPU (csrc/section.hip): the restatement of xs_layout in
tests/section_calls.py against kh_cross_sections_scratch_bytes (a host function), and the batches of the GPU file on the CPU
statement alone -- that they reach the regimes they are built for: sections beyond the LDS queue whose late arrivals share visited
bits with the small section that follows, a run of three cut voxels in one column for every dominant axis, every value of c_w & 3,
and no section beyond the queue the host sizes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_calls as S  # noqa: E402
import section_ref  # noqa: E402


def _lib():
    from kimimaro_amd import _abi, build
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


# ---- the layout -----------------------------------------------------------------------------------------------------------------------

EXTENTS = [
    (1, 1, 1), (1, 1, 9), (1, 7, 1), (5, 1, 1),                    # axes of extent one
    (1, 8, 8), (8, 8, 8), (4, 4, 4),                               # the largest face a multiple of 8
    (3, 3, 3), (7, 5, 3), (23, 23, 1),                             # and not
    (1, 1, 2048), (32, 16, 5), (2, 2, 512),                        # queue_cap == 2048 (by the volume, by 4 x face, by both): no spill
    (1, 1, 2049), (1, 3, 683),                                     # queue_cap == 2049: a spill of one word
    (27, 19, 5),                                                   # 4 x face == 2052 < nvox
    (16, 16, 8),                                                   # 2048 voxels, 4 x face == 1024
    (20, 18, 16), (24, 20, 16), (52, 50, 48), (150, 150, 6), (512, 512, 512),
    (2048, 2048, 1000), (1, 2, 2147483647),                         # just below 2^32 - 1 voxels
]
WAVES = [1, 2, 7, 20000]


@pytest.mark.parametrize("shape", EXTENTS)
def test_layout_restatement(shape):
    f = _lib().kh_cross_sections_scratch_bytes
    L = S.layout(shape)
    assert L.bitmap_words == (L.face + 7) // 8 + 1 and L.wave_bytes == 4 * (L.bitmap_words + L.spill_cap)
    for waves in WAVES:
        assert int(f(*shape, waves)) == L.scratch_bytes(waves) == 256 + waves * L.wave_bytes, (shape, waves)


def test_layout_cases_are_the_intended_ones():
    spill = {shape: S.layout(shape).spill_cap for shape in EXTENTS}
    cap = {shape: S.layout(shape).queue_cap for shape in EXTENTS}
    assert [cap[s] for s in [(1, 1, 2048), (32, 16, 5), (2, 2, 512)]] == [2048] * 3
    assert [spill[s] for s in [(1, 1, 2048), (32, 16, 5), (2, 2, 512)]] == [0] * 3
    assert [spill[s] for s in [(1, 1, 2049), (1, 3, 683)]] == [1, 1]
    assert spill[(27, 19, 5)] == 4 and cap[(16, 16, 8)] == 1024
    assert S.layout((1, 8, 8)).face % 8 == 0 and S.layout((7, 5, 3)).face % 8 != 0
    assert S.layout((4, 4, 4)).wave_bytes == 12                   # the volume of the wave-cap test
    assert S.layout((1, 2, 2147483647)).nvox == 2 ** 32 - 2


@pytest.mark.parametrize("args", [(0, 4, 4, 1), (4, -1, 4, 1), (4, 4, 0, 1), (2 ** 31, 1, 1, 1), (1, 1, 2 ** 31, 1),
                                  (65536, 65536, 1, 1), (2048, 2048, 1024, 1), (1, 1, 2 ** 32 - 1, 1), (4, 4, 4, 0), (4, 4, 4, -3)])
def test_layout_refusals(args):
    assert int(_lib().kh_cross_sections_scratch_bytes(*args)) == -1


def test_launch_layout_clips_the_waves():
    L = S.layout(S.LEAK_SHAPE)
    assert (L.face, L.bitmap_words, L.queue_cap, L.spill_cap, L.wave_bytes) == (2600, 326, 10400, 8352, 34712)
    a = S.launch_layout(S.LEAK_SHAPE, 44, 37)
    assert a.waves_used == 37 and a.bitmap_end == 256 + 4 * 37 * 326 and a.used_end == 256 + 37 * 34712 < a.scratch_bytes
    b = S.launch_layout(S.LEAK_SHAPE, 5, 37)
    assert b.waves_used == 5 and b.used_end == b.scratch_bytes
    c = S.launch_layout((4, 4, 4), 20000, 16400)
    assert c.waves_used == 16384 and c.used_end == 256 + 16384 * 12
    # a scratch one byte short of a wave more holds that wave not
    assert S.LaunchLayout(S.LEAK_SHAPE, L.scratch_bytes(3) - 1, 37).waves_used == 2


# ---- the batches, on the statement alone ----------------------------------------------------------------------------------------------

def test_large_sections_outgrow_the_lds_queue():
    """the figures of an all-ones volume; the islands lie off these planes and take nothing from them"""
    ones = np.ones(S.LEAK_SHAPE, dtype=np.uint8)
    labels = S.leak_volume()
    counts = []
    for n in S.LARGE:
        vox, _, _ = section_ref.section(ones, S.LEAK_CENTRE, n, (1, 1, 1), 1)
        counts.append(len(vox))
        assert S.statement("leak", labels, (1, 1, 1), keep=True)(S.LEAK_CENTRE, n, 1)[0] == len(vox)
    assert counts == [2472, 2574, 2681] and min(counts) > S.LDS_QUEUE
    assert [S.dominant(n, (1, 1, 1)) for n in S.LARGE] == [0, 1, 2]


def _longest_run(vox, w):
    columns = {}
    for v in np.asarray(vox).tolist():
        columns.setdefault(tuple(c for axis, c in enumerate(v) if axis != w), []).append(v[w])
    best = 0
    for cs in columns.values():
        cs = sorted(cs)
        assert cs == list(range(cs[0], cs[-1] + 1))              # the cut voxels of a column are one run
        best = max(best, len(cs))
    return best


def test_run_of_three_for_every_dominant_axis():
    small = np.ones((20, 18, 16), dtype=np.uint8)
    for w, n in enumerate(S.RUN3):
        assert S.dominant(n, (1, 1, 1)) == w
        vox, _, _ = section_ref.section(small, (10, 9, 8), n, (1, 1, 1), 1)
        assert _longest_run(vox, w) == 3
        # and in the batch, on the large volume
        big = S.statement("leak", S.leak_volume(), (1, 1, 1), keep=True).voxels(S.LEAK_CENTRE, n, 1)
        assert _longest_run(big, w) == 3


@pytest.mark.parametrize("anisotropy", S.ANISOTROPIES)
def test_leak_batch_reaches_its_regimes(anisotropy):
    labels = S.leak_volume()
    items = S.leak_items(anisotropy)
    st = S.statement("leak", labels, anisotropy, keep=True)
    L = S.layout(S.LEAK_SHAPE)
    assert 35 <= len(items) <= 45
    residues, empty, stale_followers, large = set(), 0, 0, 0
    for k, (seed, n, want) in enumerate(items):
        count = st(seed, n, want)[0]
        assert count <= L.queue_cap
        if count == 0:
            empty += 1
            continue
        w = S.dominant(n, anisotropy)
        vox = st.voxels(seed, n, want)
        assert _longest_run(vox, w) <= 4                          # what a nibble per column rests on
        residues.update(int(v[w]) & 3 for v in vox.tolist())
        if count <= S.LDS_QUEUE:
            continue
        large += 1
        # the late arrivals of this section share (column, c_w & 3) with a voxel, not the seed, of the island's section right
        # behind it: a wave that left those bits set would not count that voxel.  (Only the item right behind it: clearing is by
        # whole words, so that item wipes the island's columns for the ones after it.)
        stale = {S.visited_bit(v, w, S.LEAK_SHAPE) for v in S.surely_spilled(vox, seed)}
        assert len(stale) >= 300
        s2, n2, w2 = items[k + 1]
        if st(s2, n2, w2)[0] and S.dominant(n2, anisotropy) == w:
            hits = [v for v in st.voxels(s2, n2, w2).tolist() if tuple(v) != tuple(s2) and S.visited_bit(v, w, S.LEAK_SHAPE) in stale]
            stale_followers += len(hits) == 3
    assert residues == {0, 1, 2, 3}
    assert empty == 7 and large == 9
    assert stale_followers >= 3                                   # behind the first large section of every axis: all three others


def test_invalid_items_are_invalid_for_their_reason():
    labels = S.leak_volume()
    st = S.statement("leak", labels, (1, 1, 1), keep=True)
    bad = [(s, n, w) for s, n, w in S.leak_items() if st(s, n, w)[0] == 0]
    kinds = set()
    for s, n, w in bad:
        if s is None:
            kinds.add("outside")
        elif not np.all(np.isfinite(n)):
            kinds.add("nan")
        elif not np.any(n):
            kinds.add("zero")
        else:
            assert labels[s] != w
            kinds.add("off its label")
    assert kinds == {"outside", "nan", "zero", "off its label"}
    assert int(S.seed_lin([None], S.LEAK_SHAPE)[0]) == 0xFFFFFFFF


def test_no_other_batch_outgrows_its_queue():
    """the shell (whole and in its boxes, plain and filled), the pockets, the tube and the 4^3 volume"""
    for filled in (False, True):
        for box in [None] + S.SHELL_BOXES:
            items, want = S.shell_statement(2, filled, box)
            cap = S.layout(S.SHELL_SHAPE if box is None else box[1]).queue_cap
            assert len(items) >= 8 and 0 < max(w[0] for w in want) <= cap
    assert max(w[0] for w in S.pocket_statement(S.pocket_items())) <= S.layout(S.POCKET_SHAPE).queue_cap
    labels, items = S.symmetry_case()
    for anisotropy in S.ANISOTROPIES:
        counts = [w[0] for w in S.Statement(labels, anisotropy).batch(items)]
        assert len(items) == 16 and 0 < min(counts) and max(counts) <= S.layout(labels.shape).queue_cap
    labels, items = S.cap_case()
    assert max(w[0] for w in S.Statement(labels, (1, 1, 1)).batch(items[:6])) <= S.layout(S.CAP_SHAPE).queue_cap == 64
    assert items[6:12] == items[:6] and len(items) == S.CAP_ITEMS


def test_shell_labels_expose_a_truncating_load():
    for label_bytes, (A, B) in S.SHELL_LABELS.items():
        assert A != B and max(A, B) < 2 ** (8 * label_bytes)
        labels = S.shell_volume(label_bytes)
        assert labels.dtype.itemsize == label_bytes and set(np.unique(labels).tolist()) == {0, A, B}
        if label_bytes > 1:
            half = 2 ** (4 * label_bytes)
            assert A % half == B % half                           # the lower half of the words is the same
    for lo, shape in S.SHELL_BOXES:
        assert all(o + b <= d for o, b, d in zip(lo, shape, S.SHELL_SHAPE))
    (lo0, shape0), (lo1, shape1) = S.SHELL_BOXES
    assert lo0 == (0, 0, 0) and all(b < d for b, d in zip(shape0, S.SHELL_SHAPE))                    # flush with three faces
    assert all(o > 0 and o + b < d for o, b, d in zip(lo1, shape1, S.SHELL_SHAPE))                    # interior


def test_pocket_lists_pin_the_search():
    labels, region = S.pocket_volume()
    assert sorted(set(np.unique(region).tolist()) - {5, 65}) == S.POCKET_IDS
    assert [len(S.pocket_voxels(k)) for k in range(12)] == [1, 2, 3, 4] * 3
    for k in range(12):
        for v in S.pocket_voxels(k):
            assert labels[v] == 100 + k and region[v] == S.POCKET_IDS[k]
    assert S.POCKET_LISTS["one"] == [10] and S.POCKET_LISTS["ends"] == [10, 120] and S.POCKET_LISTS["none"] == []
    assert all(10 < r < 120 for r in S.POCKET_IDS[1:-1] + [65])        # refused by the search, not by the compare with the ends
    assert all(sorted(ids) == ids for ids in S.POCKET_LISTS.values())
    # the statement tells the lists apart on the section through the slab under every pocket
    counts = {name: w[0] for (s, n, name), w in zip(S.pocket_items(), S.pocket_statement(S.pocket_items())) if s == (20, 2, 3) and n[1] == 1.0}
    assert counts == {"one": 81, "ends": 84, "all": 107, "second": 92, "none": 80}
