"""kh_cross_sections, _filled, _box and _filled_box call by call, at wave counts the test chooses (csrc/section.hip; DESIGN.md 3.12,
3.16, 3.17).

kimimaro_amd.section sizes the scratch for one wave per item (up to 2 048), so through it a wave hardly ever takes a second item and
what it carries from item to item -- the nibble-per-column visited bitmap it clears by walking its queue again, the LDS queue and
its spill, the dominant axis and with it the numbering of the columns -- is never checked on purpose.  Here the entry points are
called through eng.lib (tests/section_calls.py) with a scratch sized for W waves, every output and the whole scratch 0xA5 with 64
guard elements behind each, and the scratch is read back: the item counter ends at n_items + waves, the overflow flag is 0, every
bitmap of a used wave is all zero again, and nothing is written behind the layout the launch uses (it clips the waves to n_items and
to 16 384 and puts the spill directly behind the clipped bitmaps).  The area is an integer sum, so every wave count gives the same
bytes.

Every comparison with the statement asks what tests/test_gpu_section.py asks: voxels equal, contact (and clip) equal, area within
the 2 float32 ulps that file derives.  tests/test_section_calls_host.py shows on the statement alone that the batches reach the
regimes they are made for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_calls as S  # noqa: E402

pytestmark = pytest.mark.gpu


def leak_call(anisotropy, waves):
    labels = S.leak_volume()
    seeds, normals, wants = S.split(S.leak_items(anisotropy))
    return S.launch(labels, anisotropy, seeds, wants, normals, waves)


def leak_want(anisotropy):
    return S.statement("leak", S.leak_volume(), anisotropy).batch(S.leak_items(anisotropy))


# ---- 1. one wave, a batch built to make state leak ------------------------------------------------------------------------------------

@pytest.mark.parametrize("anisotropy", S.ANISOTROPIES)
def test_one_wave_takes_every_item(anisotropy):
    n = len(S.leak_items())
    got = leak_call(anisotropy, 1)
    want = leak_want(anisotropy)
    assert max(w[0] for w in want) > S.LDS_QUEUE and sum(w[0] == 0 for w in want) == 7
    S.assert_outputs(got, want, "W=1 %s" % (anisotropy,))
    lay = S.launch_layout(S.LEAK_SHAPE, 1, n)
    assert lay.waves_used == 1
    S.assert_scratch_after(got.scratch, lay, n)


# ---- 2. wave-count independence -------------------------------------------------------------------------------------------------------

def test_every_wave_count_gives_the_same_bytes():
    n = len(S.leak_items())
    first = leak_call((1, 1, 1), 1)
    S.assert_outputs(first, leak_want((1, 1, 1)), "W=1")
    for waves in (1, 2, 3, 5, n, n + 7):
        got = leak_call((1, 1, 1), waves)
        assert got.rc == S.KH_OK
        assert got.area.tobytes() == first.area.tobytes(), waves
        assert np.array_equal(got.contact, first.contact) and np.array_equal(got.voxels, first.voxels), waves
        lay = S.launch_layout(S.LEAK_SHAPE, waves, n)
        assert lay.waves_used == min(waves, n)
        S.assert_scratch_after(got.scratch, lay, n)
    assert lay.used_end < lay.scratch_bytes                       # n + 7: the clipped layout was in force


# ---- 3. the same item 200 times -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["large", "run3"])
def test_one_item_two_hundred_times(which):
    normal = S.LARGE[2] if which == "large" else S.RUN3[0]
    labels = S.leak_volume()
    want = S.statement("leak", labels, (1, 1, 1))(S.LEAK_CENTRE, normal, 1)
    assert want[0] > S.LDS_QUEUE
    got = S.launch(labels, (1, 1, 1), [S.LEAK_CENTRE] * 200, [1] * 200, [normal] * 200, 3)
    area, contact, voxels = S.assert_outputs(got, [want] * 200, which)
    assert len(set(area.view(np.uint32).tolist())) == 1 and len(set(contact.tolist())) == 1 and len(set(voxels.tolist())) == 1
    S.assert_scratch_after(got.scratch, S.launch_layout(S.LEAK_SHAPE, 3, 200), 200)


# ---- 4. all twelve instantiations -----------------------------------------------------------------------------------------------------

_TABLES = {}


def shell_tables(label_bytes):
    """(region u32 [x, y, z] of the dataset, {label: (begin, count)}, the lists): section.hole_tables, once per width"""
    if label_bytes not in _TABLES:
        from kimimaro_amd import ops, section
        eng = ops.engine()
        labels = S.shell_volume(label_bytes)
        d_region, word_range, d_ids = section.hole_tables(eng, eng.to_device(labels), label_bytes, labels.shape, S.SHELL_LABELS[label_bytes])
        region = d_region.cpu().numpy().view(np.uint32).reshape(labels.shape, order="F")
        _TABLES[label_bytes] = (region, word_range, d_ids.cpu().numpy().view(np.uint32))
    return _TABLES[label_bytes]


@pytest.mark.parametrize("mode", ["plain", "filled", "box", "filled_box"])
@pytest.mark.parametrize("label_bytes", [1, 2, 4])
def test_instantiations(label_bytes, mode):
    from kimimaro_amd import ops
    filled, boxed = mode in ("filled", "filled_box"), mode in ("box", "filled_box")
    labels = S.shell_volume(label_bytes)
    A, B = S.SHELL_LABELS[label_bytes]
    an = S.SHELL_ANISOTROPY
    exponent = int(ops.engine().lib.kh_cross_sections_fixed_exponent(*S.SHELL_SHAPE, *[float(a) for a in an]))
    assert exponent != -2 ** 31
    for box in (S.SHELL_BOXES if boxed else [None]):
        items, want = S.shell_statement(label_bytes, filled, box)
        seeds, normals, wants = S.split(items)
        assert len(items) >= 8
        holes = None
        if filled:
            region, word_range, ids = shell_tables(label_bytes)
            assert word_range[A][1] >= 2 and word_range[B][1] == 0               # the cavity and B; B has no holes
            ranges = np.array([word_range[w] for w in wants], dtype=np.uint32)
            holes = (region if box is None else S.crop(region, *box), ranges[:, 0], ranges[:, 1], ids)
        if box is None:
            got = S.launch(labels, an, seeds, wants, normals, 3, holes=holes)
        else:
            got = S.launch(S.crop(labels, *box), an, seeds, wants, normals, 3, holes=holes, box=(box[0], S.SHELL_SHAPE, exponent))
        out = S.assert_outputs(got, want, "%s %d bytes %s" % (mode, label_bytes, box))
        shape = labels.shape if box is None else box[1]
        S.assert_scratch_after(got.scratch, S.launch_layout(shape, 3, len(items)), len(items))
        if box is not None and box[0] == (0, 0, 0):
            assert np.any(out[1] != 0) and np.any(out[3] != 0)                   # flush with three faces of the dataset
        elif box is not None:
            assert np.all(out[1] == 0) and np.any(out[3] != 0)                   # interior: every face it reaches is a cut
    # the core asked for the wall's label: nothing unless filled -- and something if a load dropped the upper bytes of the words
    whole_items, whole_want = S.shell_statement(label_bytes, filled, None)
    core = [w for (s, _, l), w in zip(whole_items, whole_want) if s == (11, 9, 7) and l == A]
    assert len(core) == 2 and all((w[0] > 0) == filled for w in core)


# ---- 5. hand-made hole lists ----------------------------------------------------------------------------------------------------------

def test_hand_made_hole_lists():
    labels, region = S.pocket_volume()
    items = S.pocket_items()
    want = S.pocket_statement(items)
    names = list(S.POCKET_LISTS)
    ids = np.array([r for name in names for r in S.POCKET_LISTS[name]], dtype=np.uint32)
    begin = dict(zip(names, np.cumsum([0] + [len(S.POCKET_LISTS[name]) for name in names])[:-1]))
    seeds, normals, lists = S.split(items)
    holes = (region, [begin[name] for name in lists], [len(S.POCKET_LISTS[name]) for name in lists], ids)
    wants = [S.POCKET_LABEL] * len(items)
    got = S.launch(labels, (1, 1, 1), seeds, wants, normals, 2, holes=holes)
    area, contact, voxels = S.assert_outputs(got, want, "lists")
    S.assert_scratch_after(got.scratch, S.launch_layout(S.POCKET_SHAPE, 2, len(items)), len(items))
    by = {(name, s): int(v) for (s, _, name), v in zip(items, voxels) if s[2] == 4}              # the seeds in pockets
    first, second, middle, last = (S.pocket_voxels(k)[0] for k in (0, 1, 5, 11))
    assert by["one", first] > 0 and by["one", second] == 0 and by["one", last] == 0
    assert by["ends", first] > 0 and by["ends", last] > 0 and by["ends", second] == 0 and by["ends", middle] == 0   # inside [min, max], absent
    assert all(by["all", s] > 0 for s in (first, second, middle, last))
    assert by["second", first] > 0 and by["second", second] == 0 and by["second", last] == 0
    slab = {name: int(v) for (s, n, name), v in zip(items, voxels) if s == (20, 2, 3) and n[1] == 1.0}    # the plane under every pocket
    assert slab == {"one": 81, "ends": 84, "all": 107, "second": 92, "none": 80}
    # an empty list gives the plain kernel's outputs bit for bit
    mine = [k for k, name in enumerate(lists) if name == "none"]
    plain = S.launch(labels, (1, 1, 1), [seeds[k] for k in mine], [S.POCKET_LABEL] * len(mine), [normals[k] for k in mine], 2)
    S.assert_outputs(plain, [want[k] for k in mine], "plain")
    assert plain.area[:len(mine)].tobytes() == area[mine].tobytes()
    assert np.array_equal(plain.contact[:len(mine)], contact[mine]) and np.array_equal(plain.voxels[:len(mine)], voxels[mine])


# ---- 6. exact symmetries of the arithmetic --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anisotropy", S.ANISOTROPIES)
def test_scaled_and_negated_normals(anisotropy):
    labels, items = S.symmetry_case()
    seeds, normals, wants = S.split(items)
    normals = np.array(normals)
    base = S.launch(labels, anisotropy, seeds, wants, normals, 3)
    S.assert_outputs(base, S.Statement(labels, anisotropy).batch(items), "base")
    assert base.voxels[:len(items)].min() > 0
    for name, other in (("2^-20", normals * 2.0 ** -20), ("2^20", normals * 2.0 ** 20), ("negated", -normals)):
        got = S.launch(labels, anisotropy, seeds, wants, other, 3)
        assert S.same_outputs(got, base), name
        S.assert_scratch_after(got.scratch, S.launch_layout(labels.shape, 3, len(items)), len(items))


# ---- 7. the cap of 16 384 waves -------------------------------------------------------------------------------------------------------

def test_wave_cap():
    labels, items = S.cap_case()
    n = len(items)
    assert n == 16400 > S.WAVE_CAP
    seeds, normals, wants = S.split(items)
    got = S.launch(labels, (1, 1, 1), seeds, wants, normals, 20000)
    st = S.Statement(labels, (1, 1, 1))
    want = st.batch(items)
    assert len(st.memo) == 6
    print("the six items:", want[:6])
    S.assert_outputs(got, want, "cap", show=False)
    lay = S.launch_layout(S.CAP_SHAPE, 20000, n)
    assert lay.waves_used == S.WAVE_CAP and lay.volume.wave_bytes == 12
    assert int(got.scratch[:8].view(np.uint64)[0]) == 16400 + 16384
    S.assert_scratch_after(got.scratch, lay, n)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------

SMALL_ITEMS = [((3, 2, 2), S.AXES[0], 1), ((1, 1, 1), S.AXES[2], 1)]


def _small_call(**over):
    labels = np.ones((6, 5, 4), dtype=np.uint8, order="F")
    seeds, normals, wants = S.split(SMALL_ITEMS)
    return S.launch(labels, (1, 1, 1), seeds, wants, normals, over.pop("waves", 2), **over)


def _own_exponent():
    from kimimaro_amd import ops
    e = int(ops.engine().lib.kh_cross_sections_fixed_exponent(6, 5, 4, 1.0, 1.0, 1.0))
    assert e != -2 ** 31
    return e


def test_refusals_write_nothing():
    from kimimaro_amd import _abi
    want = S.Statement(np.ones((6, 5, 4), dtype=np.uint8), (1, 1, 1)).batch(SMALL_ITEMS)
    assert [w[0] for w in want] == [20, 30]
    S.assert_outputs(_small_call(), want, "accepted")                         # the same call is accepted as it stands
    one_wave = S.layout((6, 5, 4)).scratch_bytes(1)
    e = _own_exponent()
    refused = {
        "one byte short of a wave": dict(waves=1, scratch_bytes=one_wave - 1),
        "scratch offset by 4 bytes": dict(scratch_offset=4),
        "label_bytes 8": dict(label_bytes=8),
        "fixed_exponent below the box's own": dict(box=((0, 0, 0), (6, 5, 4), e - 1)),
        "box leaves the dataset": dict(box=((1, 0, 0), (6, 5, 4), e)),
        "box at a negative origin": dict(box=((0, -1, 0), (6, 6, 4), e)),
    }
    for name, over in refused.items():
        got = _small_call(**over)
        assert got.rc == S.KH_EINVAL, name
        assert "kh_cross_sections" in _abi.last_error(), name
        S.assert_nothing_written(got)
    # accepted with the box's own exponent, so the two box refusals above are about the exponent and the origin alone
    boxed = _small_call(box=((0, 0, 0), (6, 5, 4), e))
    S.assert_outputs(boxed, [w + (0,) for w in want], "box")
    # no items: accepted, and nothing is written either -- not even the header
    for box in (None, ((0, 0, 0), (6, 5, 4), e)):
        got = _small_call(n_items=0, box=box)
        assert got.rc == S.KH_OK
        S.assert_nothing_written(got)
