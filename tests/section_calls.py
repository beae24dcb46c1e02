"""The four plane-section entry points called directly, their scratch read back, and the batches of tests/test_gpu_section_calls.py
(csrc/section.hip).  No test functions: tests/test_section_calls_host.py checks the layout restatement
and the batches on the CPU statement alone, tests/test_gpu_section_calls.py runs them on the card.

  layout / launch_layout   xs_layout and the launch's use of the scratch, restated: the launch clips the waves the scratch holds to
                           n_items and to 16 384 and lays the spill out directly behind the CLIPPED bitmaps.
  launch                   kh_cross_sections / _filled / _box / _filled_box through eng.lib on buffers this module allocates: every
                           output and the whole scratch (header included) 0xA5, 64 guard elements behind each.
  assert_scratch_after     the counter ends at n_items + waves (each wave fetches once past the end), no overflow, every bitmap of a
                           used wave all zero again, nothing written behind the clipped layout.
  assert_outputs           the guards, then what tests/test_gpu_section.py asks of every comparison with the statement (its within_ulps).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_ref  # noqa: E402

FILL = 0xA5
GUARD = 64
HEADER_BYTES = 256
LDS_QUEUE = 2048
WAVE_CAP = 16384
OUTSIDE = 0xFFFFFFFF
KH_OK, KH_EINVAL = 0, 1


# ---- the layout, restated -------------------------------------------------------------------------------------------------------------

class Layout:
    """xs_layout of a volume of extents `shape`"""

    def __init__(self, shape):
        sx, sy, sz = (int(v) for v in shape)
        self.shape = (sx, sy, sz)
        self.nvox = sx * sy * sz
        self.face = max(sx * sy, sx * sz, sy * sz)
        self.bitmap_words = (self.face + 7) // 8 + 1
        self.queue_cap = min(4 * self.face, self.nvox)
        self.spill_cap = max(self.queue_cap - LDS_QUEUE, 0)
        self.wave_bytes = 4 * (self.bitmap_words + self.spill_cap)

    def scratch_bytes(self, waves):
        """kh_cross_sections_scratch_bytes(sx, sy, sz, waves)"""
        return HEADER_BYTES + int(waves) * self.wave_bytes


def layout(shape):
    return Layout(shape)


class LaunchLayout:
    """what a launch with `scratch_bytes` of scratch and n_items items uses of it"""

    def __init__(self, shape, scratch_bytes, n_items):
        self.volume = Layout(shape)
        self.scratch_bytes = int(scratch_bytes)
        self.waves_used = min((self.scratch_bytes - HEADER_BYTES) // self.volume.wave_bytes, int(n_items), WAVE_CAP)
        self.bitmap_begin = HEADER_BYTES
        self.bitmap_end = HEADER_BYTES + 4 * self.waves_used * self.volume.bitmap_words         # the spill lies directly behind
        self.used_end = HEADER_BYTES + self.waves_used * self.volume.wave_bytes


def launch_layout(shape, waves, n_items):
    """the launch's layout in a scratch sized for `waves` waves"""
    return LaunchLayout(shape, Layout(shape).scratch_bytes(waves), n_items)


# ---- the direct caller ----------------------------------------------------------------------------------------------------------------

def seed_lin(seeds, shape):
    """[(x, y, z) or None] -> u32 linear indices x + sx (y + sy z); None is the word of a vertex outside the volume"""
    sx, sy, _ = (int(v) for v in shape)
    return np.array([OUTSIDE if s is None else int(s[0]) + sx * (int(s[1]) + sy * int(s[2])) for s in seeds], dtype=np.uint32)


class Result:
    """rc and everything the call could have written, as host arrays WITH their guards: area f32, contact u8, voxels u32, clip u8
    (box entries), each of n + GUARD elements; scratch u8, the whole allocation (scratch_bytes + 4 GUARD bytes)"""

    def outputs(self):
        return [(k, getattr(self, k)) for k in ("area", "contact", "voxels", "clip") if getattr(self, k) is not None]


def _filled(eng, nbytes):
    return eng.torch.full((int(nbytes),), FILL, dtype=eng.torch.uint8, device=eng.device)


def _up(eng, a):
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)                    # so that it has an address
    return eng.torch.from_numpy(a.view(np.uint8).copy()).to(eng.device)


def launch(labels, anisotropy, seeds, wants, normals, waves, holes=None, box=None, label_bytes=None, scratch_bytes=None,
           scratch_offset=0, n_items=None):
    """One call of an entry point: kh_cross_sections, with holes = (region u32 [x, y, z], begin, count, list) kh_cross_sections_filled,
    with box = (lo, dataset_shape, fixed_exponent) kh_cross_sections_box, with both kh_cross_sections_filled_box.  labels: an array
    [x, y, z] of 1, 2 or 4 bytes per voxel (of the BOX for the box entries); seeds: [(x, y, z) or None]; the scratch is sized for
    `waves` waves (kh_cross_sections_scratch_bytes).  label_bytes, scratch_bytes, scratch_offset (bytes added to the scratch's
    address) and n_items replace what the call would be handed: the refusals.  -> Result."""
    from kimimaro_amd import ops
    eng = ops.engine()
    P = eng.ptr
    labels = np.asarray(labels)
    sx, sy, sz = (int(v) for v in labels.shape)
    n = len(seeds)
    an = [float(a) for a in anisotropy]
    d_lab = _up(eng, labels.reshape(-1, order="F"))
    d_seed = _up(eng, seed_lin(seeds, labels.shape))
    d_want = _up(eng, np.asarray(wants, dtype=np.uint32))
    d_normals = _up(eng, np.asarray(normals, dtype=np.float64).reshape(-1, 3))
    nbytes = int(eng.lib.kh_cross_sections_scratch_bytes(sx, sy, sz, int(waves)))
    assert nbytes == Layout(labels.shape).scratch_bytes(waves)
    d_scratch = _filled(eng, nbytes + 4 * GUARD + 8)
    assert d_scratch.data_ptr() % 8 == 0
    d_area, d_contact, d_voxels = _filled(eng, 4 * (n + GUARD)), _filled(eng, n + GUARD), _filled(eng, 4 * (n + GUARD))
    d_clip = _filled(eng, n + GUARD) if box is not None else None
    args = [P(d_lab), labels.dtype.itemsize if label_bytes is None else label_bytes, sx, sy, sz, an[0], an[1], an[2],
            n if n_items is None else n_items, P(d_seed), P(d_want), P(d_normals)]
    keep = []
    if holes is not None:
        region, begin, count, ids = holes
        assert np.asarray(region).shape == labels.shape and len(begin) == n and len(count) == n
        keep = [_up(eng, np.asarray(region, dtype=np.uint32).reshape(-1, order="F")), _up(eng, np.asarray(begin, dtype=np.uint32)),
                _up(eng, np.asarray(count, dtype=np.uint32)), _up(eng, np.asarray(ids, dtype=np.uint32))]
        args += [P(t) for t in keep]
    if box is not None:
        lo, whole, exponent = box
        args += [int(lo[0]), int(lo[1]), int(lo[2]), int(whole[0]), int(whole[1]), int(whole[2]), int(exponent)]
    args += [P(d_area), P(d_contact), P(d_voxels)]
    if box is not None:
        args.append(P(d_clip))
    import ctypes as C
    args += [C.c_void_p(d_scratch.data_ptr() + scratch_offset), nbytes if scratch_bytes is None else scratch_bytes, eng.stream()]
    entry = {(False, False): eng.lib.kh_cross_sections, (True, False): eng.lib.kh_cross_sections_filled,
             (False, True): eng.lib.kh_cross_sections_box, (True, True): eng.lib.kh_cross_sections_filled_box}[holes is not None,
                                                                                                              box is not None]
    out = Result()
    out.rc = int(entry(*args))
    eng.sync()
    out.n, out.shape = n, (sx, sy, sz)
    out.scratch_bytes = nbytes if scratch_bytes is None else int(scratch_bytes)
    out.area = d_area.cpu().numpy().view(np.float32)
    out.contact = d_contact.cpu().numpy()
    out.voxels = d_voxels.cpu().numpy().view(np.uint32)
    out.clip = d_clip.cpu().numpy() if box is not None else None
    out.scratch = d_scratch.cpu().numpy()[:nbytes + 4 * GUARD]
    return out


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def assert_nothing_written(result):
    """every byte of every output and of the scratch still holds 0xA5"""
    for name, a in result.outputs():
        assert untouched(a), name
    assert untouched(result.scratch), "scratch"


def assert_scratch_after(scratch, lay, n_items):
    """scratch: the whole allocation as bytes, guard words included; lay: the LaunchLayout"""
    scratch = np.ascontiguousarray(scratch).view(np.uint8)
    assert scratch.size == lay.scratch_bytes + 4 * GUARD
    assert lay.waves_used >= 1
    header = scratch[:16].view(np.uint64)
    assert int(header[0]) == n_items + lay.waves_used, (int(header[0]), n_items, lay.waves_used)     # one fetch past the end per wave
    assert int(header[1]) == 0, "a section outgrew its queue"
    bitmaps = scratch[lay.bitmap_begin:lay.bitmap_end].view(np.uint32)
    left = np.flatnonzero(bitmaps)
    assert left.size == 0, ("visited bits left behind: (wave, word, value)",
                            [(int(i) // lay.volume.bitmap_words, int(i) % lay.volume.bitmap_words, hex(int(bitmaps[i]))) for i in left[:8]])
    behind = np.flatnonzero(scratch[lay.used_end:] != FILL)
    assert behind.size == 0, ("written behind the launch's layout, first at byte", lay.used_end + int(behind[0]))


def within_ulps(got, want64, ulps=2):
    from test_gpu_section import within_ulps as w                  # the tolerance that file derives; no other
    return w(got, want64, ulps)


def assert_outputs(result, want, label="", show=True):
    """want: per item (voxels, area float64, contact) or, for the box entries, (voxels, area float64, contact, clip).  Checks the
    guards, then voxels equal, contact (and clip) equal, area within the 2 float32 ulps of tests/test_gpu_section.py.
    -> (area, contact, voxels[, clip]) without the guards."""
    n = result.n
    assert result.rc == KH_OK, result.rc
    assert len(want) == n
    for name, a in result.outputs():
        assert a.size == n + GUARD and untouched(a[n:]), "the call wrote behind the %d elements of %s" % (n, name)
    area, contact, voxels = result.area[:n], result.contact[:n], result.voxels[:n]
    clip = result.clip[:n] if result.clip is not None else None
    for k, w in enumerate(want if show else []):
        print("%s item %d: voxels %d / %d, contact %d / %d, area %r / %r" % (label, k, voxels[k], w[0], contact[k], w[2], area[k], w[1])
              + (", clip %d / %d" % (clip[k], w[3]) if clip is not None else ""))
    for k, w in enumerate(want):
        assert int(voxels[k]) == w[0], (label, k, int(voxels[k]), w[0])
        assert int(contact[k]) == w[2], (label, k, int(contact[k]), w[2])
        if clip is not None:
            assert int(clip[k]) == w[3], (label, k, int(clip[k]), w[3])
        assert within_ulps(area[k], w[1]), (label, k, area[k], w[1])
    return (area, contact, voxels) if clip is None else (area, contact, voxels, clip)


def same_outputs(a, b):
    """bit for bit, the guards included"""
    return all(x.tobytes() == y.tobytes() for (_, x), (_, y) in zip(a.outputs(), b.outputs())) and len(a.outputs()) == len(b.outputs())


# ---- the statement, memoised ----------------------------------------------------------------------------------------------------------

class Statement:
    """section_ref.section on one (volume, anisotropy) by (seed, label, normal) -> (voxels, area float64, contact); with keep=True
    also the voxel list (the host tests look at it)"""

    def __init__(self, labels, anisotropy, keep=False):
        self.labels, self.anisotropy, self.keep = np.asarray(labels), tuple(float(a) for a in anisotropy), keep
        self.grid = section_ref.voxel_grid(self.labels.shape)
        self.memo, self.vox = {}, {}

    def key(self, seed, normal, label):
        return (None if seed is None else tuple(int(v) for v in seed), int(label), np.asarray(normal, dtype=np.float64).tobytes())

    def __call__(self, seed, normal, label):
        key = self.key(seed, normal, label)
        if key not in self.memo:
            if seed is None:
                vox, a, c = np.zeros((0, 3), dtype=np.int64), 0.0, 0
            else:
                vox, a, c = section_ref.section(self.labels, seed, normal, self.anisotropy, label, self.grid)
            self.memo[key] = (len(vox), a, c)
            if self.keep:
                self.vox[key] = vox
        return self.memo[key]

    def voxels(self, seed, normal, label):
        self(seed, normal, label)
        return self.vox[self.key(seed, normal, label)]

    def batch(self, items):
        return [self(s, n, w) for s, n, w in items]


_STATEMENTS = {}


def statement(name, labels, anisotropy, keep=False):
    """one Statement per (name, anisotropy) and process: the tests of a file share the sections they repeat"""
    key = (name, tuple(float(a) for a in anisotropy))
    if key not in _STATEMENTS or (keep and not _STATEMENTS[key].keep):
        _STATEMENTS[key] = Statement(labels, anisotropy, keep)
    return _STATEMENTS[key]


# ---- the batch that makes state leak ---------------------------------------------------------------------------------------------------

LEAK_SHAPE = (52, 50, 48)
LEAK_CENTRE = (26, 25, 24)
ANISOTROPIES = [(1, 1, 1), (4, 4, 40)]


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(v @ v)


def axis_vector(w, along, a, b):
    """`along` on axis w, a and b on the two others in ascending order"""
    v = [a, b]
    v.insert(w, along)
    return tuple(v)


# the large sections: a tilted unit normal along each axis, through the centre of the volume
LARGE = [unit(axis_vector(w, 1.0, 0.02, 0.01)) for w in range(3)]
# a run of three cut voxels along w in one column, for w = x, y, z (isotropic)
RUN3 = [unit(axis_vector(w, 1.001, 1.0, 1.0)) for w in range(3)]
AXES = [np.array(axis_vector(w, 1.0, 0.0, 0.0)) for w in range(3)]


def island(w):
    """the island of label 2 for the dominant axis w: four voxels along w (one of each c_w & 3) by 2 x 2 in the corner of the face
    across w, where the flood of a large section arrives last -- in the part of its queue that is spilled"""
    return tuple(slice(4, 8) if axis == w else slice(0, 2) for axis in range(3))


def leak_volume():
    labels = np.ones(LEAK_SHAPE, dtype=np.uint8, order="F")
    for w in range(3):
        labels[island(w)] = 2
    return labels


def corner_residue(w, anisotropy):
    """c_w & 3 of the voxel the large section of axis w cuts in the corner column (0, 0) of the face across w: the definition's
    |d| < h, no flood"""
    seed = np.array(LEAK_CENTRE)
    column = np.array([axis_vector(w, c, 0, 0) for c in range(LEAK_SHAPE[w])])
    d = section_ref.offsets(LARGE[w], anisotropy, column - seed)
    cut = np.flatnonzero(np.abs(d) < section_ref.half_width(LARGE[w], anisotropy))
    assert 1 <= cut.size <= 4
    return int(cut[0]) & 3


def leak_items(anisotropy=(1, 1, 1)):
    """[(seed or None, normal, label)], about 40: per dominant axis the large section, then at once the four small sections of that
    axis's island (one seed per value of c_w & 3, the plane across w: the other three voxels of each lie in columns the large
    section has just used), an item that is not valid between them; the three run-of-3 sections; the large ones again with the
    normal negated, each followed by oblique sections of the islands.  The first of the four is the one whose c_w & 3 is that of
    the large section's voxels in the island's columns (corner_residue: it depends on the anisotropy): clearing is by whole words,
    so the sections of the island wipe each other's columns and only the first meets what the large one left."""
    nan = np.array([np.nan, 0.0, 1.0])
    bad = [((4, 0, 0), AXES[0], 1),                     # the seed carries 2
           (None, AXES[1], 1),                          # 0xFFFFFFFF
           (LEAK_CENTRE, np.zeros(3), 1),
           (LEAK_CENTRE, nan, 1)]
    items = []
    for w in range(3):
        items.append((LEAK_CENTRE, LARGE[w], 1))
        first = corner_residue(w, anisotropy)
        for j in range(4):
            k = (first + j) % 4
            items.append((axis_vector(w, 4 + k, k % 2, k // 2), AXES[w], 2))
            if j == 1:
                items.append(bad[w])
    items.append(bad[3])
    for w in range(3):
        items.append((LEAK_CENTRE, RUN3[w], 1))
        items.append((axis_vector(w, 5, 1, 1), RUN3[(w + 1) % 3], 2))
    for w in (2, 0, 1):
        items.append((LEAK_CENTRE, -LARGE[w], 1))
        items.append((axis_vector(w, 6, 0, 1), LARGE[w], 2))
        items.append((axis_vector(w, 7, 1, 0), unit(axis_vector(w, 1.0, -0.3, 0.2)), 2))
        items.append(bad[w])
    return items


def split(items):
    return [s for s, _, _ in items], [n for _, n, _ in items], [w for _, _, w in items]


def dominant(normal, anisotropy):
    """xs_dominant: the axis with the largest |n_i| a_i, the lowest among equals"""
    return int(np.argmax(np.abs(np.asarray(normal, dtype=np.float64)) * np.asarray(anisotropy, dtype=np.float64)))


def bfs_levels(vox, seed):
    """{voxel: 26-connected distance from the seed inside the section}.  The kernel's queue is first in, first out, so it holds the
    voxels in an order of ascending level whatever the lanes' order inside a level is."""
    members = set(map(tuple, np.asarray(vox).tolist()))
    seed = tuple(int(v) for v in seed)
    level, todo = {seed: 0}, [seed]
    nbrs = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
    for v in todo:
        for i, j, k in nbrs:
            q = (v[0] + i, v[1] + j, v[2] + k)
            if q in members and q not in level:
                level[q] = level[v] + 1
                todo.append(q)
    return level


def surely_spilled(vox, seed):
    """the voxels of a section that lie behind LDS_QUEUE others in every first-in-first-out order: those with at least LDS_QUEUE
    voxels on lower levels"""
    level = bfs_levels(vox, seed)
    counts = np.bincount(list(level.values()))
    below = np.concatenate([[0], np.cumsum(counts)])          # below[l]: voxels on levels < l
    return [v for v, l in level.items() if below[l] >= LDS_QUEUE]


def visited_bit(voxel, w, shape):
    """(column, c_w & 3): the bit of the wave's bitmap that names the voxel under the dominant axis w"""
    x, y, z = (int(v) for v in voxel)
    U = shape[1] if w == 0 else shape[0]
    cu, cv, cw = (y if w == 0 else x), (y if w == 2 else z), (x, y, z)[w]
    return cu + U * cv, cw & 3


# ---- a shell, a core and a cavity: the twelve instantiations ---------------------------------------------------------------------------

SHELL_SHAPE = (24, 20, 16)
SHELL_ANISOTROPY = (4, 4, 40)
# (A, B) per label width: a load that drops the upper bytes of a label word reads A and B as one label
SHELL_LABELS = {1: (0x34, 0x35), 2: (0x1234, 0x0134), 4: (0x00051234, 0x00061234)}
# (lo, shape) of the two boxes: flush with the three low faces of the dataset; interior
SHELL_BOXES = [((0, 0, 0), (16, 14, 12)), ((6, 4, 3), (16, 13, 11))]


def shell_volume(label_bytes):
    """a wall of label A, two voxels thick, around a cavity of background that holds a core of label B with a bar that reaches the
    wall's inner face: hole(A) = the cavity and B.  A foot of A joins the wall to the face x = 0 of the dataset."""
    A, B = SHELL_LABELS[label_bytes]
    labels = np.zeros(SHELL_SHAPE, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[label_bytes], order="F")
    labels[3:21, 3:17, 2:14] = A
    labels[5:19, 5:15, 4:12] = 0
    labels[0:3, 9:12, 7:10] = A
    labels[10:14, 8:12, 6:10] = B
    labels[14:19, 9:11, 7:9] = B
    return labels


def shell_items(label_bytes):
    """[(seed in the dataset, normal, label)]: in the wall, in the cavity, in the core asked for A (nothing, unless filled) and for B,
    in the bar, outside"""
    A, B = SHELL_LABELS[label_bytes]
    oblique = unit((0.3, -0.5, 0.81))
    return [((4, 10, 8), AXES[2], A), ((4, 10, 8), oblique, A), ((19, 10, 8), AXES[1], A), ((19, 10, 8), unit((1.0, 1.0, 0.0)), A),
            ((7, 7, 6), AXES[0], A), ((7, 7, 6), oblique, A), ((11, 9, 7), AXES[2], A), ((11, 9, 7), oblique, A), ((11, 9, 7), AXES[1], B),
            ((16, 10, 8), AXES[2], B), ((16, 10, 8), unit((0.02, 0.01, 1.0)), A), ((12, 10, 13), AXES[0], A), (None, AXES[0], A)]


def items_in_box(items, lo, shape):
    """the items whose seed lies in the box, the seed in box coordinates (an outside seed stays outside)"""
    out = []
    for s, n, w in items:
        if s is None:
            out.append((s, n, w))
        elif all(o <= c < o + b for c, o, b in zip(s, lo, shape)):
            out.append((tuple(c - o for c, o in zip(s, lo)), n, w))
    return out


def crop(a, lo, shape):
    return np.asfortranarray(a[tuple(slice(o, o + b) for o, b in zip(lo, shape))])


def shell_statement(label_bytes, filled, box):
    """[(voxels, area, contact[, clip])] and the items, for the whole dataset (box None) or a box (lo, shape): section_ref.section /
    section_filled_ref's mask / section_box_ref's face bits"""
    import section_box_ref
    from section_filled_ref import filled_mask
    labels = shell_volume(label_bytes)
    items = shell_items(label_bytes)
    masks = {w: (filled_mask(labels, w) if filled else labels == w) for w in SHELL_LABELS[label_bytes]}
    if box is None:
        grid = section_ref.voxel_grid(labels.shape)
        want = []
        for s, n, w in items:
            vox, a, c = (np.zeros((0, 3)), 0.0, 0) if s is None else section_ref.section(masks[w], s, n, SHELL_ANISOTROPY, True, grid)
            want.append((len(vox), a, c))
        return items, want
    lo, shape = box
    items = items_in_box(items, lo, shape)
    want = []
    for s, n, w in items:
        want.append((0, 0.0, 0, 0) if s is None else
                    section_box_ref.section_in_box(crop(masks[w], lo, shape), lo, SHELL_SHAPE, s, n, SHELL_ANISOTROPY, True))
    return items, want


# ---- hand-made hole lists --------------------------------------------------------------------------------------------------------------

POCKET_SHAPE = (40, 6, 8)
POCKET_LABEL = 7
POCKET_IDS = [10 * (k + 1) for k in range(12)]


def pocket_voxels(k):
    """the one to four voxels of pocket k, on top of the slab"""
    x = 3 * k + 1
    return [(x, 2, 4), (x, 2, 5), (x + 1, 2, 4), (x, 3, 4)][:k % 4 + 1]


def pocket_volume():
    """(labels, region): a slab of label 7 (z = 2, 3) with twelve pockets of other labels on it; the region ids are written by hand:
    10, 20, .. 120 in the pockets, 5 in the slab, 65 -- inside [10, 120] and in no list -- in the background"""
    labels = np.zeros(POCKET_SHAPE, dtype=np.uint8, order="F")
    region = np.full(POCKET_SHAPE, 65, dtype=np.uint32, order="F")
    labels[:, :, 2:4] = POCKET_LABEL
    region[:, :, 2:4] = 5
    for k in range(12):
        for v in pocket_voxels(k):
            labels[v] = 100 + k
            region[v] = POCKET_IDS[k]
    return labels, region


POCKET_LISTS = {"one": [10], "ends": [10, 120], "all": POCKET_IDS, "second": POCKET_IDS[0::2], "none": []}


def pocket_items():
    """[(seed, normal, list name)]: seeds in the slab and in pockets (a seed in a listed pocket is valid, in any other it is not)"""
    y = np.array([0.0, 1.0, 0.0])
    tilt = unit((0.05, 1.0, 0.1))
    first, second, middle, last = pocket_voxels(0)[0], pocket_voxels(1)[0], pocket_voxels(5)[0], pocket_voxels(11)[0]
    items = []
    for name in POCKET_LISTS:
        items += [((20, 2, 3), y, name), ((20, 3, 2), y, name), ((5, 2, 2), tilt, name), ((20, 2, 3), unit((1.0, 1.0, 0.2)), name),
                  (first, y, name), (second, y, name), (middle, tilt, name), (last, y, name)]
    return items


def pocket_statement(items):
    labels, region = pocket_volume()
    grid = section_ref.voxel_grid(labels.shape)
    masks = {name: (labels == POCKET_LABEL) | np.isin(region, ids) for name, ids in POCKET_LISTS.items()}
    out = []
    for s, n, name in items:
        vox, a, c = section_ref.section(masks[name], s, n, (1, 1, 1), True, grid)
        out.append((len(vox), a, c))
    return out


# ---- symmetries, and the cap of 16 384 waves -------------------------------------------------------------------------------------------

def symmetry_case():
    """(labels, [(seed, normal, 1)]): 16 items on a tube, lattice and random normals"""
    from shapes import random_walk_tube
    labels = np.asfortranarray((random_walk_tube((32, 28, 24), 4) != 0).astype(np.uint8))
    rng = np.random.default_rng(12)
    normals = [unit(v) for v in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, -1), (0, 1, 1), (1, 1, 1), (1, -1, 1)]]
    normals += [unit(v) for v in rng.normal(size=(8, 3))]
    where = np.argwhere(labels != 0)
    seeds = where[rng.integers(0, len(where), size=16)]
    return labels, [(tuple(int(c) for c in s), n, 1) for s, n in zip(seeds, normals)]


CAP_SHAPE = (4, 4, 4)
CAP_ITEMS = 16400


def cap_case():
    """(labels, [(seed, normal, label)] x 16 400, cycling through six)"""
    labels = np.ones(CAP_SHAPE, dtype=np.uint8, order="F")
    labels[0, 0, :] = 0
    labels[3, 3, 3] = 2
    six = [((2, 2, 2), AXES[0], 1), ((1, 2, 1), AXES[2], 1), ((2, 1, 2), unit((1.0, 1.0, 1.0)), 1), ((3, 3, 3), AXES[1], 2),
           ((0, 0, 1), AXES[0], 1), ((1, 1, 1), unit((0.3, -0.5, 0.81)), 1)]
    return labels, [six[k % 6] for k in range(CAP_ITEMS)]
