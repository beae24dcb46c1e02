"""cross_sectional_area_filled (the reference's cross_sectional_area(fill_holes=True)) on the MI355X against the CPU statement
(tests/section_filled_ref.py): the sections of filled(L) = L and its holes.

Every comparison with the statement asks for what tests/test_gpu_section.py asks: `voxels` equal, `contact` equal, `area` within 2
float32 ulps of the statement's float64 sum rounded to float32 (both sides sum float64 per-voxel areas of relative error ~1e-15 and
round once; the kernel's fixed point quantum is far below half an ulp; 1 ulp for landing on opposite sides of a rounding boundary,
1 for margin)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_ref  # noqa: E402
import section_ref  # noqa: E402
from section_filled_ref import filled_mask  # noqa: E402
from shapes import random_walk_tube, voronoi_labels  # noqa: E402

pytestmark = pytest.mark.gpu

AXES = [(1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0)]
OBLIQUE = [tuple(np.array(v) / np.sqrt(np.dot(v, v))) for v in ((1.0, 1.0, 0.0), (0.3, -0.5, 0.81))]


def within_ulps(got, want64, ulps=2):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)


def device_sections(labels, seeds, normals, wants, anisotropy=(1, 1, 1), filled=True, stats=None):
    """kimimaro_amd.section.cross_sections on a numpy volume, through kh_cross_sections_filled with the tables of Engine.region_graph
    and kh_host_enclosed_regions (filled) or through kh_cross_sections: (area, contact, voxels)"""
    from kimimaro_amd import ops, section, utility
    eng = ops.engine()
    d_flat, itemsize, _, shape, _, span = utility._device_labels(eng, labels)
    wants = [int(w) for w in wants]
    d_lab, label_bytes, device_label = utility._narrow_labels(eng, d_flat, itemsize, span, set(wants))
    words = np.array([device_label.get(w, 0xFFFFFFFF) for w in wants], dtype=np.uint32)
    tables = None
    if filled:
        d_region, word_range, d_hole_regions = section.hole_tables(eng, d_lab, label_bytes, shape, device_label.values(), stats)
        ranges = np.array([word_range.get(int(w), (0, 0)) for w in words], dtype=np.uint32).reshape(-1, 2)
        tables = (d_region, ranges[:, 0], ranges[:, 1], d_hole_regions)
    return section.cross_sections(eng, d_lab, label_bytes, shape, anisotropy, section.seed_index(seeds, shape), words, normals,
                                  filled=tables)


def statement(labels, seeds, normals, wants, anisotropy=(1, 1, 1), filled=True):
    """[(voxels, area float64, contact)] per item"""
    labels = np.asarray(labels)
    grid = section_ref.voxel_grid(labels.shape)
    masks, memo, out = {}, {}, []
    for seed, n, w in zip(seeds, normals, wants):
        w = int(w)
        if w not in masks:
            masks[w] = filled_mask(labels, w) if filled else labels == w
        key = (tuple(int(v) for v in seed), w, np.asarray(n, dtype=np.float64).tobytes())
        if key not in memo:
            vox, a, c = section_ref.section(masks[w], seed, n, anisotropy, True, grid)
            memo[key] = (len(vox), a, c)
        out.append(memo[key])
    return out


def assert_matches_statement(labels, seeds, normals, wants, anisotropy=(1, 1, 1)):
    area, contact, voxels = device_sections(labels, seeds, normals, wants, anisotropy)
    want = statement(labels, seeds, normals, wants, anisotropy)
    for k, (seed, n, w) in enumerate(zip(seeds, normals, wants)):
        print("item %d: voxels %d / %d, contact %d / %d, area %r / %r" % (k, voxels[k], want[k][0], contact[k], want[k][2], area[k], want[k][1]))
        assert int(voxels[k]) == want[k][0], (k, seed, n, w)
        assert int(contact[k]) == want[k][2], (k, seed, n, w)
        assert within_ulps(area[k], want[k][1]), (k, seed, n, w, area[k], want[k][1])
    return (area, contact, voxels), want


def same_outputs(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _box_wall(cc, lo, hi, value):
    cc[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = value
    cc[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = 0


# ---- the kernel, item by item ----------------------------------------------------------------------------------------------------

def shell_with_core(dtype=np.uint32, shell_id=5, blob_id=9):
    """24^3: a box wall of thickness 2 (Chebyshev distance 7, 8 from the centre) around a cavity with background and a blob"""
    labels = np.zeros((24, 24, 24), dtype=dtype, order="F")
    labels[fill_ref.shell(labels.shape, (12, 12, 12), 8, 2, cube=True)] = shell_id
    labels[10:15, 10:15, 10:15] = blob_id
    seeds = [(12, 12, 20), (12, 12, 16), (12, 12, 12)]            # in the wall, in the cavity's background, in the blob
    items = [(s, n) for s in seeds for n in AXES + OBLIQUE]
    return labels, [s for s, _ in items], [n for _, n in items]


def test_shell_with_a_core():
    labels, seeds, normals = shell_with_core()
    wants = [5] * len(seeds)
    got, want = assert_matches_statement(labels, seeds, normals, wants)
    plain = statement(labels, seeds, normals, wants, filled=False)
    assert any(w[0] > p[0] > 0 for w, p in zip(want, plain))                          # a wall seed: an annulus becomes a disc
    assert all(p[0] == 0 for p, s in zip(plain, seeds) if s != (12, 12, 20))          # a cavity seed: nothing becomes a disc
    assert all(w[0] > 0 for w in want)
    unfilled = device_sections(labels, seeds, normals, wants, filled=False)
    assert np.all(unfilled[2][5:] == 0) and np.all(got[2][5:] > 0)                    # the cavity seeds
    assert np.all(unfilled[2][:5] <= got[2][:5]) and np.any(unfilled[2][:5] < got[2][:5])


@pytest.mark.parametrize("ids", [(3, 7), (7, 3)])
def test_nested_shells(ids):
    """shell A around shell B around a core, and a label without holes, in one launch"""
    A, B = ids
    labels = np.zeros((28, 28, 28), dtype=np.uint32, order="F")
    labels[fill_ref.shell(labels.shape, (14, 14, 14), 11, 2, cube=True)] = A
    labels[fill_ref.shell(labels.shape, (14, 14, 14), 6, 2, cube=True)] = B
    labels[13:16, 13:16, 13:16] = 11
    labels[0:3, 0:3, 0:8] = 20
    spots = [(14, 14, 24), (14, 14, 22), (14, 14, 19), (14, 14, 17), (14, 14, 14)]     # A's wall, between, B's wall, B's cavity, core
    seeds, normals, wants = [], [], []
    for want in (A, B, 20):
        for s in spots + [(1, 1, 4)]:
            for n in [AXES[0], AXES[2], OBLIQUE[1]]:
                seeds.append(s), normals.append(n), wants.append(want)
    got, want = assert_matches_statement(labels, seeds, normals, wants)
    wants = np.array(wants)
    by = lambda L, s: [w[0] for w, x, y in zip(want, wants, seeds) if x == L and y == s]
    assert min(by(A, spots[4])) > 0 and min(by(B, spots[4])) > 0             # the core lies in both holes
    assert min(by(A, spots[2])) > 0 and max(by(B, spots[1])) == 0            # B lies in A's; the gap between them is not B's
    unfilled = device_sections(labels, seeds, normals, wants, filled=False)
    third = wants == 20
    assert got[2][third].max() > 0
    assert same_outputs([g[third] for g in got], [u[third] for u in unfilled])


def test_open_shells_have_no_holes():
    normals = AXES + OBLIQUE
    gap = np.zeros((20, 20, 20), dtype=np.uint16, order="F")
    _box_wall(gap, (4, 4, 4), (15, 15, 15), 6)
    gap[10, 10, 15] = 0                                                       # a one-voxel gap in the wall
    cut = np.zeros((20, 20, 20), dtype=np.uint16, order="F")
    _box_wall(cut, (4, 4, 0), (15, 15, 9), 6)
    cut[5:15, 5:15, 0] = 0                                                    # no wall on the volume's face: the inside touches it
    for labels, seeds in ((gap, [(10, 10, 10), (10, 4, 10)]), (cut, [(10, 10, 5), (10, 4, 5)])):
        items = [(s, n) for s in seeds for n in normals]
        args = (labels, [s for s, _ in items], [n for _, n in items], [6] * len(items))
        got, _ = assert_matches_statement(*args)
        assert same_outputs(got, device_sections(*args, filled=False))
        assert got[2].max() > 0
    gap[10, 10, 15] = 6                                                       # closed: the same items differ
    items = [(s, n) for s in [(10, 10, 10), (10, 4, 10)] for n in normals]
    args = (gap, [s for s, _ in items], [n for _, n in items], [6] * len(items))
    got, _ = assert_matches_statement(*args)
    unfilled = device_sections(*args, filled=False)
    assert np.all(unfilled[2][:5] == 0) and np.all(got[2][:5] > 0)            # the seed in the cavity
    assert np.all(got[2][5:] >= unfilled[2][5:]) and np.any(got[2][5:] > unfilled[2][5:])


@pytest.mark.parametrize("shell_id, thread_id", [(4, 9), (9, 4)])
def test_thread_crossing_a_shell_diagonally(shell_id, thread_id):
    """a 26-connected thread replaces a voxel of the shell's edge: no 6-connected way in, so the part inside belongs to the shell's
    filled set, the part outside does not"""
    cc = np.zeros((16, 16, 12), dtype=np.uint32, order="F")
    _box_wall(cc, (2, 2, 2), (8, 8, 8), shell_id)
    for k in range(5, 11):
        cc[k, k, 5] = thread_id
    cc[10:13, 10:13, 4:7] = thread_id
    cc[11, 11, 5] = 0
    inside, outside = [(5, 5, 5), (7, 7, 5)], [(8, 8, 5), (9, 9, 5)]
    seeds = [s for s in inside + outside for _ in range(3)]
    normals = [AXES[2], AXES[0], OBLIQUE[0]] * 4
    got, want = assert_matches_statement(cc, seeds, normals, [shell_id] * len(seeds))
    assert np.all(got[2][:6] > 0) and np.all(got[2][6:] == 0)
    # the thread's own sections, and its own hole at (11, 11, 5)
    assert_matches_statement(cc, [(11, 11, 5), (9, 9, 5), (6, 6, 5)], [AXES[2]] * 3, [thread_id] * 3)


def test_section_beyond_the_lds_queue():
    """72^3, a hollow box of wall 2: each filled section through the centre has thousands of voxels, far beyond the 2 048 entries of
    the LDS queue, so the spill path runs with region lookups"""
    from kimimaro_amd import ops
    labels = np.zeros((72, 72, 72), dtype=np.uint8, order="F")
    labels[fill_ref.shell(labels.shape, (36, 36, 36), 33, 2, cube=True)] = 3
    normals = [AXES[2], tuple(np.array([0.02, 0.01, 1.0]) / np.sqrt(0.02 ** 2 + 0.01 ** 2 + 1.0))]
    seeds = [(36, 36, 36)] * 2
    got, want = assert_matches_statement(labels, seeds, normals, [3, 3])
    assert got[2].min() >= 67 * 67 > 2 * 2048
    assert np.all(device_sections(labels, seeds, normals, [3, 3], filled=False)[2] == 0)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64])
def test_label_widths(dtype):
    big = {1: 0, 2: 40000, 4: 3 * 10 ** 9, 8: 2 ** 40}[np.dtype(dtype).itemsize]
    shell_id, blob_id = (big + 5, big + 9) if np.dtype(dtype).kind == "u" else (-5, 9)
    labels, seeds, normals = shell_with_core(dtype, shell_id, blob_id)
    got, want = assert_matches_statement(labels, seeds, normals, [shell_id] * len(seeds))
    assert all(w[0] > 0 for w in want)


def test_extent_one_axis():
    """every voxel of a (20, 20, 1) volume lies on a face: a ring has no hole"""
    labels = np.zeros((20, 20, 1), dtype=np.uint8, order="F")
    labels[4:16, 4:16, 0] = 2
    labels[6:14, 6:14, 0] = 0
    seeds = [(10, 10, 0), (5, 10, 0)] * 2
    normals = [AXES[2]] * 2 + [OBLIQUE[1]] * 2
    got, _ = assert_matches_statement(labels, seeds, normals, [2] * 4)
    assert same_outputs(got, device_sections(labels, seeds, normals, [2] * 4, filled=False))
    assert got[2][0] == 0 and got[2][1] > 0


def test_skewed_batch_and_edge_items():
    labels, _, _ = shell_with_core()
    labels[0:4, 0:4, :] = 2                                                   # a bar without holes
    rng = np.random.default_rng(7)
    seeds, normals, wants = [], [], []
    for k in range(300):
        if k % 3 == 0:
            seeds.append((1 + k % 2, 2, int(rng.integers(0, 24)))), normals.append(AXES[2]), wants.append(2)
        else:
            seeds.append(tuple(int(v) for v in rng.integers(4, 21, 3))), normals.append(tuple(rng.normal(size=3))), wants.append(5)
    edge = [((24, 3, 3), AXES[0], 5), ((-1, 3, 3), AXES[0], 5), ((12, 12, 12), (0.0, 0, 0), 5), ((12, 12, 12), (np.nan, 0, 1), 5),
            ((12, 12, 12), (np.inf, 0, 0), 5), ((1, 20, 20), AXES[0], 5), ((12, 12, 12), AXES[0], 2), ((12, 12, 12), AXES[0], 77)]
    for s, n, w in edge:                 # outside, degenerate normals, off filled(5), in 5's hole but asked for 2, an absent label
        seeds.append(s), normals.append(n), wants.append(w)
    got, want = assert_matches_statement(labels, seeds, np.array(normals, dtype=np.float64), wants)
    assert np.all(got[0][300:] == 0) and np.all(got[1][300:] == 0) and np.all(got[2][300:] == 0)
    assert got[2][:300].min() > 0 and got[2][:300].max() >= 100
    again = device_sections(labels, seeds, np.array(normals, dtype=np.float64), wants)
    assert same_outputs(got, again)


def test_empty_batch():
    labels, _, _ = shell_with_core()
    area, contact, voxels = device_sections(labels, np.zeros((0, 3), dtype=int), np.zeros((0, 3)), [])
    assert area.shape == (0,) and area.dtype == np.float32
    assert contact.shape == (0,) and contact.dtype == np.uint8
    assert voxels.shape == (0,) and voxels.dtype == np.uint32


def test_null_tables_are_refused():
    from kimimaro_amd import _abi, ops
    eng = ops.engine()
    t = eng.torch
    d_lab = t.ones(64, dtype=t.uint8, device=eng.device)
    d = t.zeros(64, dtype=t.int32, device=eng.device)
    d_normal = t.ones(3, dtype=t.float64, device=eng.device)
    nbytes = int(eng.lib.kh_cross_sections_scratch_bytes(4, 4, 4, 1))
    d_scratch = t.zeros((nbytes + 7) // 8, dtype=t.int64, device=eng.device)
    P = eng.ptr
    good = [P(d_lab), 1, 4, 4, 4, 1.0, 1.0, 1.0, 1, P(d), P(d), P(d_normal), P(d), P(d), P(d), P(d), P(d), P(d), P(d), P(d_scratch), nbytes,
            eng.stream()]
    for at in (12, 13, 14, 15):
        args = list(good)
        args[at] = None
        assert eng.lib.kh_cross_sections_filled(*args) == 1, at              # KH_EINVAL
        assert "kh_cross_sections_filled" in _abi.last_error()
        args[8] = 0
        assert eng.lib.kh_cross_sections_filled(*args) == 0, at              # an empty batch reads nothing


# ---- the driver ------------------------------------------------------------------------------------------------------------------

def _walk_points(shape, seed, steps, step, radius):
    """the centres random_walk_tube visits (its generator, replayed)"""
    rng = np.random.default_rng(seed)
    p = np.array([shape[0] / 2, shape[1] / 2, shape[2] / 2], dtype=np.float64)
    d = rng.normal(size=3)
    out = []
    for _ in range(steps):
        d = d + 0.7 * rng.normal(size=3)
        d /= np.linalg.norm(d) + 1e-9
        p = np.clip(p + step * d, 1, np.array(shape) - 2)
        rng.uniform(*radius)
        out.append(p.copy())
    return out


def _voxel_path(points):
    """a 26-connected voxel path through the rounded points"""
    path = [tuple(int(v) for v in np.round(points[0]))]
    for q in points[1:]:
        q = np.round(q).astype(int)
        while path[-1] != tuple(q):
            here = np.array(path[-1])
            path.append(tuple(int(v) for v in here + np.clip(q - here, -1, 1)))
    return path


_TUBE = {}
TUBE, FILLING, BAR = 4, 2, 6


def tube_case():
    """(labels, {id: (vertices in voxels, edges)}, the voxels of the voids' centres): a tube with spherical voids carved along its
    axis, every other one filled with another label; its skeleton is the axis, so vertices lie inside voids.  A bar without holes
    is the second object."""
    if not _TUBE:
        shape, args = (44, 40, 36), dict(steps=24, step=3.0, radius=(3.0, 4.5))
        mask = random_walk_tube(shape, 11, **args)
        points = _walk_points(shape, 11, **args)
        labels = np.zeros(shape, dtype=np.uint16, order="F")
        labels[mask != 0] = TUBE
        grid = section_ref.voxel_grid(shape)
        assert all(mask[tuple(int(v) for v in np.round(p))] for p in points), "the walk was not replayed"
        centres = []
        for k, p in enumerate(points[2::4]):
            c = np.round(p).astype(int)
            labels[np.sum((grid - c) ** 2, axis=-1) <= 2] = FILLING if k % 2 else 0
            centres.append(tuple(int(v) for v in c))
        path = _voxel_path(points)
        free = labels[:, 1:4, 1:4] == 0
        labels[:, 1:4, 1:4][free] = BAR
        skels = {TUBE: (np.array(path), np.array([[i, i + 1] for i in range(len(path) - 1)])),
                 BAR: (np.array([[x, 2, 2] for x in range(44)]), np.array([[x, x + 1] for x in range(43)]))}
        _TUBE["case"] = (labels, skels, centres)
        _TUBE["sections"] = {}
    return _TUBE["case"]


def tube_sections(label, anisotropy, filled=True):
    key = (label, tuple(anisotropy), filled)
    if key not in _TUBE["sections"]:
        labels = tube_case()[0]
        _TUBE["sections"][key] = section_ref.SectionCache(filled_mask(labels, label) if filled else labels == label, anisotropy)
    return _TUBE["sections"][key]


def fresh(skels, space, anisotropy):
    from kimimaro_amd import Skeleton
    scale = np.array(anisotropy, dtype=np.float32) if space == "physical" else np.ones(3, dtype=np.float32)
    return {k: Skeleton(v.astype(np.float32) * scale, e.copy(), segid=k, space=space) for k, (v, e) in skels.items()}


def assert_skeleton_matches(skel, want_area, want_contact):
    assert skel.cross_sectional_area.dtype == np.float32 and skel.cross_sectional_area_contacts.dtype == np.uint8
    assert len(skel.cross_sectional_area) == len(skel.vertices) == len(skel.cross_sectional_area_contacts)
    assert np.array_equal(skel.cross_sectional_area_contacts, want_contact)
    ok = within_ulps(skel.cross_sectional_area, want_area)
    assert np.all(ok), (np.flatnonzero(~ok), skel.cross_sectional_area[~ok], want_area[~ok])


@pytest.mark.parametrize("container", ["dict", "list", "single"])
@pytest.mark.parametrize("space", ["physical", "voxel"])
@pytest.mark.parametrize("anisotropy", [(1, 1, 1), (2, 2, 5)])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("smoothing_window", [1, 3])
def test_driver_tube_with_voids(smoothing_window, step, anisotropy, space, container):
    import kimimaro_amd
    labels, skels, centres = tube_case()
    mine = fresh(skels, space, anisotropy)
    if container == "dict":
        out = kimimaro_amd.cross_sectional_area_filled(labels, mine, anisotropy, smoothing_window, step=step)
        assert out is mine
    elif container == "list":
        arg = list(mine.values())
        out = kimimaro_amd.cross_sectional_area_filled(labels, arg, anisotropy, smoothing_window, step=step)
        assert out is arg
    else:
        mine = {TUBE: mine[TUBE]}
        out = kimimaro_amd.cross_sectional_area_filled(labels, mine[TUBE], anisotropy, smoothing_window, step=step)
        assert out is mine[TUBE]
    for k, s in mine.items():
        want_area, want_contact = section_ref.single_skeleton(tube_sections(k, anisotropy), labels.shape, s.vertices, s.edges, space,
                                                              True, anisotropy, smoothing_window, step)
        assert_skeleton_matches(s, want_area, want_contact)
    if step == 1:
        # the vertices inside the voids: an area with fill_holes=True, 0 without
        plain = kimimaro_amd.cross_sectional_area(labels, fresh(skels, space, anisotropy)[TUBE], anisotropy, smoothing_window)
        in_void = np.array([labels[tuple(v)] != TUBE for v in skels[TUBE][0]])
        assert in_void.sum() >= len(centres)
        assert np.all(plain.cross_sectional_area[in_void] == 0)
        assert np.count_nonzero(mine[TUBE].cross_sectional_area[in_void] > 0) >= len(centres) // 2


def _bar_with_voids():
    """a bar of 8 x 8 voxels along x (label 7) with 2^3 voids on its axis, every other one holding label 3, and a skeleton that
    wobbles along the axis through them"""
    from kimimaro_amd import Skeleton
    bar = np.zeros((60, 20, 20), dtype=np.uint16, order="F")
    bar[:, 6:14, 6:14] = 7
    for k, x in enumerate(range(4, 56, 6)):
        bar[x:x + 2, 9:11, 9:11] = 3 if k % 2 else 0
    vertices = np.array([[x, 9 + (x // 5) % 2, 10] for x in range(60)])
    edges = np.array([[x, x + 1] for x in range(59)])
    return bar, Skeleton(vertices, edges, segid=7)


def test_multipass_over_two_halves():
    """two volumes, one skeleton: the second pass re-evaluates what the first left at 0, with the second volume's tables"""
    import kimimaro_amd
    bar, line = _bar_with_voids()
    low, high = bar.copy(order="F"), bar.copy(order="F")
    low[33:] = 0
    high[:29] = 0
    stats = {}
    kimimaro_amd.cross_sectional_area_filled(low, line, multipass=True)
    first = line.cross_sectional_area.copy()
    kimimaro_amd.cross_sectional_area_filled(high, line, multipass=True, _stats=stats)
    print("second pass:", {k: v for k, v in stats.items() if k in ("rounds", "launches", "items", "vertices")})
    lo_sec = section_ref.SectionCache(filled_mask(low, 7), (1, 1, 1))
    hi_sec = section_ref.SectionCache(filled_mask(high, 7), (1, 1, 1))
    a, c = section_ref.single_skeleton(lo_sec, low.shape, line.vertices, line.edges, "physical", True, (1, 1, 1))
    assert np.array_equal(first == 0, a == 0)
    a, c = section_ref.single_skeleton(hi_sec, high.shape, line.vertices, line.edges, "physical", True, (1, 1, 1), areas=a, contacts=c)
    assert_skeleton_matches(line, a, c)
    in_void = bar[tuple(line.vertices.astype(int).T)] != 7
    assert in_void[:29].any() and in_void[33:].any()
    assert np.all(first[33:] == 0) and np.all(line.cross_sectional_area > 0)


def test_repair_contacts_after_widening():
    import kimimaro_amd
    bar, line = _bar_with_voids()
    crop = np.asfortranarray(bar[:29])                     # cuts the void at x = 28, 29 open
    kimimaro_amd.cross_sectional_area_filled(crop, line)
    before_area, before_contact = line.cross_sectional_area.copy(), line.cross_sectional_area_contacts.copy()
    crop_sec = section_ref.SectionCache(filled_mask(crop, 7), (1, 1, 1))
    a, c = section_ref.single_skeleton(crop_sec, crop.shape, line.vertices, line.edges, "physical", True, (1, 1, 1))
    assert_skeleton_matches(line, a, c)
    assert np.any(before_contact[:29] & 2) and np.any(before_contact[1:29] == 0) and before_area[28] == 0
    kimimaro_amd.cross_sectional_area_filled(bar, line, repair_contacts=True)
    whole_sec = section_ref.SectionCache(filled_mask(bar, 7), (1, 1, 1))
    a, c = section_ref.single_skeleton(whole_sec, bar.shape, line.vertices, line.edges, "physical", True, (1, 1, 1),
                                       areas=before_area.copy(), contacts=before_contact.copy(), repair_contacts=True)
    assert_skeleton_matches(line, a, c)
    whole = kimimaro_amd.cross_sectional_area_filled(bar, _bar_with_voids()[1])
    assert np.array_equal(line.cross_sectional_area, whole.cross_sectional_area)
    assert np.array_equal(line.cross_sectional_area_contacts, whole.cross_sectional_area_contacts)
    assert np.all(whole.cross_sectional_area > 0)


def test_input_forms():
    import torch
    import kimimaro_amd
    from kimimaro_amd import Skeleton, ops
    labels, skels, _ = tube_case()
    a = kimimaro_amd.cross_sectional_area_filled(labels, fresh(skels, "voxel", (1, 1, 1)))
    tensor = torch.from_numpy(labels.astype(np.int64)).to(ops.engine().device)
    b = kimimaro_amd.cross_sectional_area_filled(tensor, fresh(skels, "voxel", (1, 1, 1)))
    for k in a:
        assert np.any(a[k].cross_sectional_area > 0)
        assert np.array_equal(a[k].cross_sectional_area, b[k].cross_sectional_area)
        assert np.array_equal(a[k].cross_sectional_area_contacts, b[k].cross_sectional_area_contacts)
    # a bool volume gives every skeleton label 1: the voids that hold another label are holes of the mask too
    mask = np.asfortranarray(labels == TUBE)
    s = fresh(skels, "voxel", (1, 1, 1))[TUBE]
    s.id = 424242
    kimimaro_amd.cross_sectional_area_filled(mask, s)
    assert np.array_equal(s.cross_sectional_area, a[TUBE].cross_sectional_area)
    # the skip rules look at the label as given
    v, e = skels[TUBE]
    lonely = labels.copy(order="F")
    lonely[43, 39, 35] = 555
    arg = [Skeleton(v.copy(), e.copy(), segid=777), Skeleton(v.copy(), e.copy(), segid=0),
           Skeleton(np.array([[43, 39, 35], [42, 39, 35]]), np.array([[0, 1]]), segid=555), fresh(skels, "voxel", (1, 1, 1))[TUBE]]
    kimimaro_amd.cross_sectional_area_filled(lonely, arg, step=2)
    kimimaro_amd.cross_sectional_area_filled(lonely, arg)
    for s in arg[:3]:
        assert s.cross_sectional_area.dtype == np.float32 and np.all(s.cross_sectional_area == -1)
        assert s.cross_sectional_area_contacts.dtype == np.uint8 and np.all(s.cross_sectional_area_contacts == 0)
    for s in arg:
        ids = [p["id"] for p in s.extra_attributes]
        assert ids.count("cross_sectional_area") == 1 and ids.count("cross_sectional_area_contacts") == 1
    assert np.array_equal(arg[3].cross_sectional_area, a[TUBE].cross_sectional_area)


def test_volume_without_holes():
    import kimimaro_amd
    from kimimaro_amd import Skeleton
    labels = voronoi_labels((32, 32, 32), 8, 5)
    assert all(np.array_equal(filled_mask(labels, L), labels == L) for L in np.unique(labels))
    skels = kimimaro_amd.skeletonize(labels, dust_threshold=100, progress=False)
    assert len(skels) >= 4
    copy = lambda: {k: Skeleton(s.vertices.copy(), s.edges.copy(), segid=k, space="physical") for k, s in skels.items()}
    stats = {}
    a = kimimaro_amd.cross_sectional_area_filled(labels, copy(), smoothing_window=3, _stats=stats)
    b = kimimaro_amd.cross_sectional_area(labels, copy(), smoothing_window=3)
    assert stats["holes"]["csr_regions"] == 0 and stats["holes"]["labels_with_holes"] == 0
    for k in a:
        assert np.any(a[k].cross_sectional_area > 0)
        assert a[k].cross_sectional_area.tobytes() == b[k].cross_sectional_area.tobytes()
        assert np.array_equal(a[k].cross_sectional_area_contacts, b[k].cross_sectional_area_contacts)


def test_unrelated_raises_stay():
    import kimimaro_amd
    labels, skels, _ = tube_case()
    with pytest.raises(NotImplementedError, match="fill_holes"):
        kimimaro_amd.oversegment(labels, fresh(skels, "voxel", (1, 1, 1)), fill_holes=True)
    with pytest.raises(NotImplementedError):
        kimimaro_amd.cross_sectional_area_filled(labels, fresh(skels, "voxel", (1, 1, 1)), visualize_section_planes=True)
    # the keyword of cross_sectional_area keeps raising (tests/test_section_host.py) and names the function that is the option
    with pytest.raises(NotImplementedError, match="cross_sectional_area_filled"):
        kimimaro_amd.cross_sectional_area(labels, fresh(skels, "voxel", (1, 1, 1)), fill_holes=True)
