"""cross_sectional_area on the MI355X against the CPU statement (tests/section_ref.py).

Every comparison with the statement asks for: `voxels` equal, `contact` equal, `area` within 2 float32 ulps of the statement's
float64 sum rounded to float32 (both sides sum float64 per-voxel areas of relative error ~1e-15 and round once; the kernel's fixed
point quantum is far below half an ulp; 1 ulp for landing on opposite sides of a rounding boundary, 1 for margin).  Closed forms
are asked for exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_ref  # noqa: E402
from shapes import random_walk_tube, voronoi_labels  # noqa: E402

pytestmark = pytest.mark.gpu

LATTICE = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1),
           (1, -1, 1), (-1, 1, 1)]
NEAR = [(1, 1e-9, 0), (0, 1, 1e-9), (1e-9, 0, 1), (1, 1, 1e-9), (1, -1e-7, 1e-7)]


def normals64(seed):
    """64 unit normals: the 13 lattice directions, near-degenerate ones, random ones"""
    rng = np.random.default_rng(seed)
    out = [np.array(v, dtype=np.float64) for v in LATTICE + NEAR]
    out += list(rng.normal(size=(64 - len(out), 3)))
    return np.stack([v / np.sqrt(v @ v) for v in out])


def within_ulps(got, want64, ulps=2):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)


def device_sections(labels, seeds, normals, wants, anisotropy=(1, 1, 1)):
    """kimimaro_amd.section.cross_sections on a numpy volume: (area, contact, voxels)"""
    from kimimaro_amd import ops, section, utility
    eng = ops.engine()
    d_flat, itemsize, _, shape, _, span = utility._device_labels(eng, labels)
    wants = [int(w) for w in wants]
    d_lab, label_bytes, device_label = utility._narrow_labels(eng, d_flat, itemsize, span, set(wants))
    words = np.array([device_label.get(w, 0xFFFFFFFF) for w in wants], dtype=np.uint32)
    return section.cross_sections(eng, d_lab, label_bytes, shape, anisotropy, section.seed_index(seeds, shape), words, normals)


def assert_matches_statement(labels, seeds, normals, wants, anisotropy=(1, 1, 1), memo=None):
    area, contact, voxels = device_sections(labels, seeds, normals, wants, anisotropy)
    grid = section_ref.voxel_grid(np.asarray(labels).shape)
    for k, (seed, n, w) in enumerate(zip(seeds, normals, wants)):
        key = (tuple(int(v) for v in seed), int(w), np.asarray(n, dtype=np.float64).tobytes())
        if memo is None or key not in memo:
            vox, a, c = section_ref.section(labels, seed, n, anisotropy, w, grid)
            if memo is not None:
                memo[key] = (len(vox), a, c)
            want = (len(vox), a, c)
        else:
            want = memo[key]
        print("item %d: voxels %d / %d, contact %d / %d, area %r / %r" % (k, voxels[k], want[0], contact[k], want[2], area[k], want[1]))
        assert int(voxels[k]) == want[0], (k, seed, n)
        assert int(contact[k]) == want[2], (k, seed, n)
        assert within_ulps(area[k], want[1]), (k, seed, n, area[k], want[1])
    return area, contact, voxels


def foreground_seeds(labels, count, seed):
    rng = np.random.default_rng(seed)
    where = np.argwhere(np.asarray(labels) != 0)
    return where[rng.integers(0, len(where), size=count)]


# ---- reference KATs ------------------------------------------------------------------------------------------------------------

def test_reference_line():
    """automated_test.py:512-527"""
    import kimimaro_amd
    labels = np.ones((100, 3, 3), dtype=bool, order="F")
    vertices = np.array([[x, 1, 1] for x in range(100)])
    edges = np.array([[x, x + 1] for x in range(99)])
    skel = kimimaro_amd.Skeleton(vertices, edges, segid=1)
    out = kimimaro_amd.cross_sectional_area(labels, skel, smoothing_window=5)
    assert out is skel
    assert len(skel.cross_sectional_area) == 100
    assert np.all(skel.cross_sectional_area == 9)
    want = np.full(100, 60)
    want[0], want[99] = 61, 62
    assert np.array_equal(skel.cross_sectional_area_contacts, want)


def test_reference_cube_steps():
    """automated_test.py:588-604 on 40^3"""
    import kimimaro_amd
    labels = np.ones((40, 40, 40), dtype=np.uint8)
    skel = kimimaro_amd.skeletonize(labels, teasar_params={"pdrf_exponent": 16}, progress=False)[1]
    xsa_1 = kimimaro_amd.cross_sectional_area(labels, skel, step=1).cross_sectional_area.copy()
    xsa_10 = kimimaro_amd.cross_sectional_area(labels, skel, step=10).cross_sectional_area.copy()
    assert np.all(xsa_1[xsa_10 == 0] != xsa_10[xsa_10 == 0])
    assert np.all(xsa_1[xsa_10 > 0] == xsa_10[xsa_10 > 0])
    terminals = skel.terminals()
    assert len(terminals) >= 2
    assert np.all(xsa_10[terminals] > 0)


# ---- exact closed forms --------------------------------------------------------------------------------------------------------

def test_closed_forms_anisotropic_cube():
    from kimimaro_amd import ops
    labels = np.ones((9, 9, 9), dtype=np.uint8)
    assert ops.cross_sectional_area(labels, (4, 4, 4), (1, 0, 0), (4, 4, 40), return_contact=True) == (81.0 * 160, 60)
    assert ops.cross_sectional_area(labels, (4, 4, 4), (0, 0, 1), (4, 4, 40), return_contact=True) == (81.0 * 16, 15)
    assert ops.cross_sectional_area(labels, (4, 4, 4), (0, 0, 1), (4, 4, 40)) == 81.0 * 16


def test_closed_form_hexagon():
    from kimimaro_amd import ops
    labels = np.ones((21, 21, 21), dtype=bool)
    area, contact = ops.cross_sectional_area(labels, (10, 10, 10), np.ones(3) / np.sqrt(3.0), return_contact=True)
    print("hexagon", area, 3 * np.sqrt(3.0) / 4 * 441)
    assert within_ulps(area, 3 * np.sqrt(3.0) / 4 * 441)
    assert contact == 63


# ---- single points against the statement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("anisotropy", [(1, 1, 1), (4, 4, 40), (40, 4, 4)])
def test_tube_points(anisotropy):
    labels = random_walk_tube((48, 40, 36), 4)
    normals = normals64(1)
    seeds = foreground_seeds(labels, 64, 2)
    assert_matches_statement(labels, seeds, normals, np.ones(64, dtype=int), anisotropy)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])
def test_voronoi_points(dtype):
    labels = voronoi_labels((40, 36, 32), 12, 6)
    if dtype == np.uint8:
        labels = (labels - 1000 + 1).astype(np.uint8)
    elif dtype == np.uint16:
        labels = (labels + 40000).astype(np.uint16)
    elif dtype == np.uint64:
        labels = labels.astype(np.uint64) + np.uint64(2 ** 40)
    else:
        labels = labels.astype(np.uint32) + np.uint32(3 * 10 ** 9)
    labels = np.asfortranarray(labels)
    normals = normals64(3)
    seeds = foreground_seeds(labels, 64, 4)
    wants = [int(labels[tuple(s)]) for s in seeds]
    _, _, voxels = assert_matches_statement(labels, seeds, normals, wants)
    assert voxels.max() < 40 * 36 * 3        # sections stop at other labels


def test_tensor_input_equals_numpy():
    import torch
    import kimimaro_amd
    from kimimaro_amd import ops
    labels = random_walk_tube((48, 40, 36), 4)
    tensor = torch.from_numpy(np.ascontiguousarray(labels)).to(ops.engine().device)
    normals = normals64(5)[:8]
    seeds = foreground_seeds(labels, 8, 6)
    for seed, n in zip(seeds, normals):
        assert ops.cross_sectional_area(tensor, seed, n, (4, 4, 40), True) == ops.cross_sectional_area(labels, seed, n, (4, 4, 40), True)
    lab = voronoi_labels((40, 36, 32), 12, 6)
    skels = kimimaro_amd.skeletonize(lab, dust_threshold=100, progress=False)
    a = kimimaro_amd.cross_sectional_area(lab, fresh(skels, "physical", (1, 1, 1)), smoothing_window=3)
    b = kimimaro_amd.cross_sectional_area(torch.from_numpy(lab.astype(np.int64)).to(ops.engine().device),
                                          fresh(skels, "physical", (1, 1, 1)), smoothing_window=3)
    assert len(a) >= 8
    for k in a:
        assert np.any(a[k].cross_sectional_area > 0)
        assert np.array_equal(a[k].cross_sectional_area, b[k].cross_sectional_area)
        assert np.array_equal(a[k].cross_sectional_area_contacts, b[k].cross_sectional_area_contacts)


# ---- connectivity ----------------------------------------------------------------------------------------------------------------

def test_only_the_bar_with_the_vertex():
    labels = np.zeros((20, 12, 5), dtype=np.uint8, order="F")
    labels[:, 1:4, 1:4] = 1
    labels[:, 7:10, 1:4] = 1
    area, contact, voxels = assert_matches_statement(labels, [(10, 2, 2)], [(1.0, 0, 0)], [1])
    assert voxels[0] == 9 and area[0] == 9 and contact[0] == 0


def test_only_the_arm_of_the_u():
    labels = np.zeros((18, 12, 5), dtype=np.uint8, order="F")
    labels[:16, 1:4, 1:4] = 1
    labels[:16, 7:10, 1:4] = 1
    labels[13:16, 1:10, 1:4] = 1
    area, contact, voxels = assert_matches_statement(labels, [(5, 8, 2), (5, 2, 2), (14, 5, 2)], [(1.0, 0, 0)] * 3, [1] * 3)
    assert voxels.tolist() == [9, 9, 27] and area.tolist() == [9, 9, 27]


def test_grazed_voxel_does_not_bridge():
    """n = (1, 1, 0) / sqrt 2: a voxel at offset (1, 0, .) has |d| == h exactly -- the plane touches one of its edges"""
    s = 1 / np.sqrt(2.0)
    n = np.array([s, s, 0.0])
    assert section_ref.offsets(n, (1, 1, 1), np.array([1, 0, 1])) == section_ref.half_width(n, (1, 1, 1))
    labels = np.zeros((12, 12, 6), dtype=np.uint8, order="F")
    labels[5, 5, 1] = 1          # A, the seed
    labels[6, 5, 2] = 1          # grazed: touches A and B
    labels[6, 4, 3] = 1          # B: cut, and not a neighbour of A
    area, contact, voxels = assert_matches_statement(labels, [(5, 5, 1), (6, 4, 3)], [n] * 2, [1] * 2)
    assert voxels.tolist() == [1, 1]
    labels[6, 4, 2] = 1          # a cut voxel between them joins them
    _, _, voxels = assert_matches_statement(labels, [(5, 5, 1)], [n], [1])
    assert voxels.tolist() == [3]


# ---- sizes where the kernel can go wrong -----------------------------------------------------------------------------------------

BIG_NORMAL = np.array([0.02, 0.01, 1.0]) / np.sqrt(0.02 ** 2 + 0.01 ** 2 + 1.0)


def test_section_larger_than_any_queue():
    labels = np.ones((150, 150, 6), dtype=np.uint8)
    _, _, voxels = assert_matches_statement(labels, [(75, 75, 3)], [BIG_NORMAL], [1])
    assert voxels[0] >= 22500


@pytest.mark.parametrize("shape", [(130, 3, 3), (65, 67, 3)])
def test_rows_across_the_wave_boundary(shape):
    labels = np.ones(shape, dtype=np.uint8)
    normals = np.stack([v / np.sqrt(v @ v) for v in np.array([(0, 0, 1.0), (0, 1.0, 0), (1.0, 0, 0), (0.01, 0.02, 1), (0.01, 1, 0.02), (1, 1, 1)])])
    centre = tuple(s // 2 for s in shape)
    assert_matches_statement(labels, [centre] * len(normals), normals, [1] * len(normals))


def test_seeds_on_faces_and_corner():
    labels = np.ones((9, 8, 7), dtype=np.uint8)
    seeds = [(0, 4, 3), (8, 4, 3), (4, 0, 3), (4, 7, 3), (4, 4, 0), (4, 4, 6), (0, 0, 0), (8, 7, 6)]
    normals = normals64(9)[[0, 2, 9, 12, 13, 20, 30]]
    for n in normals:
        assert_matches_statement(labels, seeds, [n] * len(seeds), [1] * len(seeds), (4, 4, 40))


def _mixed_batch():
    labels = np.zeros((150, 150, 10), dtype=np.uint8, order="F")
    labels[:, :, :6] = 1
    labels[:, 1:4, 7:10] = 2
    seeds = [(10 + 13 * (k % 10), 2, 8) for k in range(3001)]
    normals = [np.array([1.0, 0, 0])] * 3001
    wants = [2] * 3001
    seeds[1500], normals[1500], wants[1500] = (75, 75, 3), BIG_NORMAL, 1
    return labels, seeds, normals, wants


def test_skewed_batch():
    labels, seeds, normals, wants = _mixed_batch()
    area, contact, voxels = assert_matches_statement(labels, seeds, normals, wants, memo={})
    assert voxels[1500] >= 22500 and np.all(np.delete(voxels, 1500) == 9)
    again = device_sections(labels, seeds, normals, wants)
    assert area.tobytes() == again[0].tobytes() and np.array_equal(contact, again[1]) and np.array_equal(voxels, again[2])


def test_empty_batch():
    labels = np.ones((5, 5, 5), dtype=np.uint8)
    area, contact, voxels = device_sections(labels, np.zeros((0, 3), dtype=int), np.zeros((0, 3)), [])
    assert area.shape == (0,) and area.dtype == np.float32
    assert contact.shape == (0,) and contact.dtype == np.uint8
    assert voxels.shape == (0,) and voxels.dtype == np.uint32


def test_empty_sections():
    labels = np.zeros((8, 8, 8), dtype=np.uint8, order="F")
    labels[2:6, 2:6, 2:6] = 1
    seeds = [(0, 0, 0), (9, 3, 3), (-1, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3)]
    normals = [(1, 0, 0), (1, 0, 0), (1, 0, 0), (0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0), (1, 0, 0)]
    wants = [1, 1, 1, 1, 1, 1, 2]
    area, contact, voxels = assert_matches_statement(labels, seeds, np.array(normals, dtype=np.float64), wants)
    assert np.all(area == 0) and np.all(contact == 0) and np.all(voxels == 0)


# ---- the driver against the statement's sequential loop --------------------------------------------------------------------------

_DRIVER = {}


def driver_case(anisotropy):
    """(labels, skeletons in physical space, SectionCache) for voronoi_labels((48, 44, 40), 10, .): made once per anisotropy"""
    if anisotropy not in _DRIVER:
        import kimimaro_amd
        labels = voronoi_labels((48, 44, 40), 10, 8, anisotropy=anisotropy)
        skels = kimimaro_amd.skeletonize(labels, anisotropy=anisotropy, dust_threshold=100, progress=False)
        assert len(skels) >= 8
        _DRIVER[anisotropy] = (labels, skels, section_ref.SectionCache(labels, anisotropy))
    return _DRIVER[anisotropy]


def fresh(skels, space, anisotropy):
    from kimimaro_amd import Skeleton
    out = {}
    for k, s in skels.items():
        v = s.vertices if space == "physical" else s.vertices / np.array(anisotropy, dtype=np.float32)
        out[k] = Skeleton(v.copy(), s.edges.copy(), segid=k, space=space)
    return out


def assert_skeleton_matches(skel, want_area, want_contact):
    assert skel.cross_sectional_area.dtype == np.float32 and skel.cross_sectional_area_contacts.dtype == np.uint8
    assert len(skel.cross_sectional_area) == len(skel.vertices) == len(skel.cross_sectional_area_contacts)
    assert np.array_equal(skel.cross_sectional_area_contacts, want_contact)
    ok = within_ulps(skel.cross_sectional_area, want_area)
    assert np.all(ok), (np.flatnonzero(~ok), skel.cross_sectional_area[~ok], want_area[~ok])


@pytest.mark.parametrize("container", ["dict", "list", "single"])
@pytest.mark.parametrize("space", ["physical", "voxel"])
@pytest.mark.parametrize("anisotropy", [(1, 1, 1), (4, 4, 40)])
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("smoothing_window", [1, 5])
def test_driver(smoothing_window, step, anisotropy, space, container):
    import kimimaro_amd
    labels, skels, sections = driver_case(anisotropy)
    mine = fresh(skels, space, anisotropy)
    if container == "dict":
        out = kimimaro_amd.cross_sectional_area(labels, mine, anisotropy, smoothing_window, step=step)
        assert out is mine
    elif container == "list":
        arg = list(mine.values())
        out = kimimaro_amd.cross_sectional_area(labels, arg, anisotropy, smoothing_window, step=step)
        assert out is arg
    else:
        mine = {k: mine[k] for k in list(mine)[:1]}
        arg = next(iter(mine.values()))
        out = kimimaro_amd.cross_sectional_area(labels, arg, anisotropy, smoothing_window, step=step)
        assert out is arg
    evaluated = 0
    for k, s in mine.items():
        want_area, want_contact = section_ref.single_skeleton(sections, labels.shape, s.vertices, s.edges, space, k, anisotropy,
                                                              smoothing_window, step)
        assert_skeleton_matches(s, want_area, want_contact)
        evaluated += int((want_area > 0).sum())
    assert evaluated > 0


def test_driver_skips():
    import kimimaro_amd
    from kimimaro_amd import Skeleton
    labels, skels, sections = driver_case((1, 1, 1))
    mine = fresh(skels, "physical", (1, 1, 1))
    first = next(iter(mine))
    absent = Skeleton(mine[first].vertices.copy(), mine[first].edges.copy(), segid=77777, space="physical")
    zero = Skeleton(mine[first].vertices.copy(), mine[first].edges.copy(), segid=0, space="physical")
    lonely = labels.copy()
    lonely[0, 0, 0] = 55555
    single = Skeleton(np.array([[0, 0, 0], [1, 0, 0]]), np.array([[0, 1]]), segid=55555, space="physical")
    arg = [absent, zero, single, mine[first]]
    kimimaro_amd.cross_sectional_area(lonely, arg)
    for s in arg[:3]:
        assert s.cross_sectional_area.dtype == np.float32 and np.all(s.cross_sectional_area == -1)
        assert s.cross_sectional_area_contacts.dtype == np.uint8 and np.all(s.cross_sectional_area_contacts == 0)
        assert len(s.cross_sectional_area) == len(s.vertices)
        assert [a["id"] for a in s.extra_attributes].count("cross_sectional_area") == 1
    assert np.any(mine[first].cross_sectional_area > 0)


def test_driver_bool_volume():
    import kimimaro_amd
    labels, skels, _ = driver_case((1, 1, 1))
    first = next(iter(skels))
    mask = np.asfortranarray(labels == first)
    sections = section_ref.SectionCache(mask, (1, 1, 1))
    s = fresh(skels, "physical", (1, 1, 1))[first]
    s.id = 424242                                    # a bool volume gives every skeleton label 1
    kimimaro_amd.cross_sectional_area(mask, s)
    want_area, want_contact = section_ref.single_skeleton(sections, mask.shape, s.vertices, s.edges, "physical", True, (1, 1, 1))
    assert_skeleton_matches(s, want_area, want_contact)


def _longest(skels):
    return max(skels, key=lambda k: np.ptp(skels[k].vertices[:, 0]))


def test_multipass_over_two_halves():
    import kimimaro_amd
    labels, skels, sections = driver_case((1, 1, 1))
    k = _longest(skels)
    s = fresh(skels, "physical", (1, 1, 1))[k]
    whole = kimimaro_amd.cross_sectional_area(labels, fresh(skels, "physical", (1, 1, 1))[k])
    mask = labels == k
    xs = np.round(s.vertices[:, 0]).astype(int)
    cut = int(np.median(xs))
    low, high = np.asfortranarray(mask[:cut + 2]), np.asfortranarray(mask[cut - 2:])
    kimimaro_amd.cross_sectional_area_single(low, s, None, multipass=True)
    kimimaro_amd.cross_sectional_area_single(high, s, (cut - 2, 0, 0), multipass=True)
    # the statement, through the same two passes
    lo_sec, hi_sec = section_ref.SectionCache(low, (1, 1, 1)), section_ref.SectionCache(high, (1, 1, 1))
    a, c = section_ref.single_skeleton(lo_sec, low.shape, s.vertices, s.edges, "physical", True, (1, 1, 1))
    a, c = section_ref.single_skeleton(hi_sec, high.shape, s.vertices, s.edges, "physical", True, (1, 1, 1), offset=(cut - 2, 0, 0),
                                       areas=a, contacts=c)
    assert_skeleton_matches(s, a, c)
    # a section that touches neither cut face is the whole volume's
    branch = set(s.branches().tolist())
    clean = [i for i in range(len(xs)) if i not in branch and ((xs[i] < cut - 2 and not s.cross_sectional_area_contacts[i] & 2)
                                                               or (xs[i] >= cut + 2 and not s.cross_sectional_area_contacts[i] & 1))]
    assert len(clean) >= 4
    assert np.array_equal(s.cross_sectional_area[clean], whole.cross_sectional_area[clean])


def test_repair_contacts_after_widening():
    import kimimaro_amd
    labels, skels, sections = driver_case((1, 1, 1))
    k = _longest(skels)
    s = fresh(skels, "physical", (1, 1, 1))[k]
    xs = np.round(s.vertices[:, 0]).astype(int)
    cut = int(np.median(xs)) + 1
    crop = np.asfortranarray(labels[:cut])
    kimimaro_amd.cross_sectional_area(crop, s)
    before_area, before_contact = s.cross_sectional_area.copy(), s.cross_sectional_area_contacts.copy()
    assert np.any(before_contact & 2)
    crop_sec = section_ref.SectionCache(crop, (1, 1, 1))
    a, c = section_ref.single_skeleton(crop_sec, crop.shape, s.vertices, s.edges, "physical", k, (1, 1, 1))
    assert_skeleton_matches(s, a, c)
    kimimaro_amd.cross_sectional_area(labels, s, repair_contacts=True)
    a, c = before_area.copy(), before_contact.copy()          # the second pass starts from the skeleton's arrays
    a, c = section_ref.single_skeleton(sections, labels.shape, s.vertices, s.edges, "physical", k, (1, 1, 1), areas=a, contacts=c,
                                       repair_contacts=True)
    assert_skeleton_matches(s, a, c)
    # on a bar that keeps clear of the volume's walls: the contacts the crop caused are gone, the other vertices keep their areas
    bar, line = _bar()
    kimimaro_amd.cross_sectional_area(np.asfortranarray(bar[:30]), line)
    cropped_area, cropped_contact = line.cross_sectional_area.copy(), line.cross_sectional_area_contacts.copy()
    assert np.all(cropped_area[30:] == 0) and np.any(cropped_contact[:30] & 2) and np.any(cropped_contact[1:30] == 0)
    kimimaro_amd.cross_sectional_area(bar, line, repair_contacts=True)
    whole = kimimaro_amd.cross_sectional_area(bar, _bar()[1])
    assert np.array_equal(line.cross_sectional_area, whole.cross_sectional_area)
    assert np.array_equal(line.cross_sectional_area_contacts, whole.cross_sectional_area_contacts)
    keep = np.flatnonzero(cropped_contact[:30] == 0)
    assert np.array_equal(line.cross_sectional_area[keep], cropped_area[keep])


def _bar():
    """a bar of 8 x 8 voxels along x with a margin to the y and z walls, and a skeleton that wobbles along its axis"""
    from kimimaro_amd import Skeleton
    bar = np.zeros((60, 20, 20), dtype=np.uint16, order="F")
    bar[:, 6:14, 6:14] = 7
    vertices = np.array([[x, 9 + (x // 5) % 2, 10] for x in range(60)])
    edges = np.array([[x, x + 1] for x in range(59)])
    return bar, Skeleton(vertices, edges, segid=7)


def test_branch_point_is_the_mean():
    import kimimaro_amd
    from kimimaro_amd import Skeleton
    labels = np.zeros((40, 40, 9), dtype=np.uint8, order="F")
    verts, edges = [], []
    for x in range(2, 20):                      # stem along x
        verts.append((x, 20, 4))
    for t in range(1, 15):                      # two arms
        verts.append((19 + t, 20 + t, 4))
    for t in range(1, 15):
        verts.append((19 + t, 20 - t, 4))
    stem_end = 17
    edges = [(i, i + 1) for i in range(17)] + [(stem_end, 18)] + [(i, i + 1) for i in range(18, 31)] + [(stem_end, 32)] + \
            [(i, i + 1) for i in range(32, 45)]
    for x, y, z in verts:
        labels[x - 2:x + 3, y - 2:y + 3, z - 2:z + 3] = 1
    skel = Skeleton(np.array(verts), np.array(edges), segid=1)
    assert skel.branches().tolist() == [stem_end]
    kimimaro_amd.cross_sectional_area(labels, skel)
    sections = section_ref.SectionCache(labels, (1, 1, 1))
    want_area, want_contact = section_ref.single_skeleton(sections, labels.shape, skel.vertices, skel.edges, "voxel", 1, (1, 1, 1))
    assert_skeleton_matches(skel, want_area, want_contact)
    # explicitly: the branch point occurs once per path, with that path's normal
    paths = skel.paths(return_indices=True)
    assert len(paths) == 2
    values = []
    for p in paths:
        i = p.tolist().index(stem_end)
        n = (skel.vertices[p[i + 1]] - skel.vertices[p[i]]).astype(np.float32)
        n = n / np.linalg.norm(n)
        values.append(sections(verts[stem_end], n.astype(np.float64), 1)[0])
    assert values[0] != values[1]
    mean = np.float32(np.float32(values[0] + values[1]) / np.float32(2))
    assert within_ulps(skel.cross_sectional_area[stem_end], mean)


def test_single_with_roi_offset():
    import kimimaro_amd
    labels, skels, _ = driver_case((4, 4, 40))
    k = _longest(skels)
    class Roi:
        minpt = np.array([6, 5, 3])

    crop = np.asfortranarray((labels == k)[6:42, 5:40, 3:36])
    s = fresh(skels, "physical", (4, 4, 40))[k]
    out = kimimaro_amd.cross_sectional_area_single(crop, s, Roi(), (4, 4, 40), 3)
    assert out is s
    sections = section_ref.SectionCache(crop, (4, 4, 40))
    a, c = section_ref.single_skeleton(sections, crop.shape, s.vertices, s.edges, "physical", True, (4, 4, 40), 3, offset=Roi.minpt)
    assert_skeleton_matches(s, a, c)
    # a section that touches no face of the crop is the whole volume's
    bar, line = _bar()
    whole = kimimaro_amd.cross_sectional_area(bar, _bar()[1], smoothing_window=3)
    kimimaro_amd.cross_sectional_area_single(np.asfortranarray((bar == 7)[6:50, 2:18, 3:19]), line, (6, 2, 3), smoothing_window=3)
    assert np.all(line.cross_sectional_area[:6] == 0) and np.all(line.cross_sectional_area[50:] == 0)
    free = (line.cross_sectional_area_contacts == 0) & (line.cross_sectional_area > 0)
    assert free.sum() >= 30
    assert np.array_equal(line.cross_sectional_area[free], whole.cross_sectional_area[free])


def test_attributes_once():
    import kimimaro_amd
    labels, skels, _ = driver_case((1, 1, 1))
    mine = fresh(skels, "physical", (1, 1, 1))
    kimimaro_amd.cross_sectional_area(labels, mine)
    kimimaro_amd.cross_sectional_area(labels, mine, step=2)
    for s in mine.values():
        ids = [a["id"] for a in s.extra_attributes]
        assert ids.count("cross_sectional_area") == 1 and ids.count("cross_sectional_area_contacts") == 1
        attrs = {a["id"]: a for a in s.extra_attributes}
        assert attrs["cross_sectional_area"]["data_type"] == "float32" and attrs["cross_sectional_area_contacts"]["data_type"] == "uint8"
        assert s.cross_sectional_area.dtype == np.float32 and s.cross_sectional_area_contacts.dtype == np.uint8
        assert len(s.cross_sectional_area) == len(s.vertices) == len(s.cross_sectional_area_contacts)
