"""cross_sectional_area_chunked without a GPU: the planning helpers on numbers, the host C function that chooses the
fixed point against its formula, and the driver's bookkeeping -- which sections go to which box in which round, the doubling of the
halo, bit 64 -- with the statement (tests/section_box_ref.py) in place of the kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_box_ref as B  # noqa: E402
import section_ref  # noqa: E402

SHAPES = [(64, 56, 48), (97, 5, 1), (40, 33)]
CHUNK = (16, 16, 16)


def three(shape):
    return (tuple(shape) + (1,))[:3]


# ---- plan.halo_boxes, plan.core_of ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("halo", [1, 4, 100])
@pytest.mark.parametrize("shape", SHAPES)
def test_halo_boxes_and_core_of(shape, halo):
    from kimimaro_amd import plan
    chunk = CHUNK[:len(shape)]
    core_lo, core_hi, box_lo, box_hi = plan.halo_boxes(shape, chunk, halo)
    grid = plan.chunk_grid(shape, chunk, overlap=0)
    assert np.array_equal(core_lo, grid.core_lo) and np.array_equal(core_hi, grid.core_hi)
    for a in (core_lo, core_hi, box_lo, box_hi):
        assert a.dtype == np.int64 and a.shape == (len(core_lo), 3)
    extent = np.array(three(shape), dtype=np.int64)
    # the cores partition the dataset: every voxel lies in exactly one, and core_of names it
    owner = np.full(three(shape), -1, dtype=np.int64)
    covered = np.zeros(three(shape), dtype=np.int64)
    for k, (lo, hi) in enumerate(zip(core_lo, core_hi)):
        assert np.all(lo < hi)
        owner[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = k
        covered[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
    assert np.all(covered == 1)
    vox = section_ref.voxel_grid(three(shape)).reshape(-1, 3)
    assert np.array_equal(plan.core_of(vox, shape, chunk), owner.reshape(-1))
    outside = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [extent[0], 0, 0], [0, extent[1], 0], [0, 0, extent[2]]])
    assert np.all(plan.core_of(outside, shape, chunk) == -1)
    # a box is its core widened by the halo on all six sides, clamped
    assert np.array_equal(box_lo, np.maximum(core_lo - halo, 0)) and np.array_equal(box_hi, np.minimum(core_hi + halo, extent))
    assert np.all(box_lo >= 0) and np.all(box_hi <= extent)
    if halo == 100:
        assert np.all(box_lo == 0) and np.all(box_hi == extent)
    else:
        assert np.any(box_hi - box_lo < extent)


def test_halo_boxes_refuses_a_negative_halo():
    from kimimaro_amd import plan
    with pytest.raises(ValueError):
        plan.halo_boxes((8, 8, 8), (4, 4, 4), -1)


# ---- kh_cross_sections_fixed_exponent ------------------------------------------------------------------------------------------------

def exponent(shape, anisotropy):
    """the formula, restated: e with ((ax ay + ay az) + ax az) * min(4 * largest face, voxels) < 2^e"""
    sx, sy, sz = (int(v) for v in shape)
    ax, ay, az = (float(v) for v in anisotropy)
    most = min(4 * max(sx * sy, sx * sz, sy * sz), sx * sy * sz)
    return int(np.frexp(((ax * ay + ay * az) + ax * az) * float(most))[1])


@pytest.mark.parametrize("anisotropy", [(1, 1, 1), (4, 4, 40)])
@pytest.mark.parametrize("shape", [(48, 44, 40), (64, 56, 48), (4096, 4096, 1024)])
def test_fixed_exponent(shape, anisotropy):
    from kimimaro_amd import _abi
    got = _abi.lib().kh_cross_sections_fixed_exponent(*shape, *[float(a) for a in anisotropy])
    print(shape, anisotropy, got)
    assert got == exponent(shape, anisotropy)
    assert 3.0 * min(anisotropy) ** 2 * min(4 * shape[0] * shape[1], shape[0] * shape[1] * shape[2]) < 2.0 ** got


def test_fixed_exponent_refuses():
    from kimimaro_amd import _abi
    f = _abi.lib().kh_cross_sections_fixed_exponent
    assert 4096 * 4096 * 1024 == 2 ** 34
    for bad in [(0, 4, 4, 1.0, 1.0, 1.0), (4, 4, 2 ** 31, 1.0, 1.0, 1.0), (4, 4, 4, 0.0, 1.0, 1.0), (4, 4, 4, 1.0, float("nan"), 1.0),
                (4, 4, 4, 1e300, 1e300, 1e300)]:
        assert f(*bad) == -2 ** 31


# ---- the driver's bookkeeping ----------------------------------------------------------------------------------------------------------

def bar_dataset():
    """(labels, skeletons): label 7 is a bar of 12 x 12 voxels along x across the y cut at 16, its skeleton a line along the axis; label 9
    a blob of 4^3 inside the first core with a skeleton of two vertices; label 5 occupies one voxel, 77 none"""
    from kimimaro_amd import Skeleton
    lab = np.zeros((40, 30, 20), dtype=np.uint16, order="F")
    lab[:, 10:22, 4:16] = 7
    lab[2:6, 2:6, 2:6] = 9
    lab[30, 2, 18] = 5
    line = np.array([[x, 15, 10] for x in range(2, 38)])
    edges = np.array([[i, i + 1] for i in range(len(line) - 1)])
    skels = {7: Skeleton(line, edges, segid=7, space="voxel"),
             9: Skeleton(np.array([[3, 3, 3], [4, 3, 3]]), np.array([[0, 1]]), segid=9, space="voxel"),
             5: Skeleton(np.array([[30, 2, 18], [31, 2, 18]]), np.array([[0, 1]]), segid=5, space="voxel"),
             77: Skeleton(np.array([[3, 3, 3], [4, 3, 3]]), np.array([[0, 1]]), segid=77, space="voxel")}
    return lab, skels


def whole_volume(lab, skels):
    sections = section_ref.SectionCache(lab, (1, 1, 1))
    return {k: section_ref.single_skeleton(sections, lab.shape, s.vertices, s.edges, "voxel", k, (1, 1, 1)) for k, s in skels.items()
            if k in (7, 9)}


def test_driver_rounds_with_the_statement_as_launcher():
    from kimimaro_amd import plan, post
    lab, skels = bar_dataset()
    fake, timings = B.FakeSections(), {}
    out = post.cross_sectional_area_chunked(lab, skels, chunk_shape=CHUNK, halo=2, timings=timings, _sections=fake)
    assert out is skels
    # every section of the bar leaves its box in y at halo 2 and 4 and fits at 8; the blob's fit at once
    assert timings["cores"] == 12 and len(timings["calls"]) == 1
    assert timings["calls"][0] == {"boxes": [12, 3, 3], "items": [36 + 3 * 2, 36, 36]}
    assert timings["items"] == 42 and timings["items_rerun"] == 72 and timings["capped_items"] == 0 and timings["boxes_loaded"] == 18
    assert len(fake.calls) == 18
    for r, (calls, halo) in enumerate([(fake.calls[:12], 2), (fake.calls[12:15], 4), (fake.calls[15:], 8)]):
        core_lo, core_hi, box_lo, box_hi = plan.halo_boxes(lab.shape, CHUNK, halo)
        seen = []
        for lo, ext, seeds in calls:
            k = [tuple(b) for b in box_lo.tolist()].index(lo) if r == 0 else \
                int(plan.core_of([np.array(seeds[0])], lab.shape, CHUNK)[0])
            seen.append(k)
            assert lo == tuple(box_lo[k]) and ext == tuple(box_hi[k] - box_lo[k])
            for seed in seeds:
                assert seed is None or np.all((np.array(seed) >= core_lo[k]) & (np.array(seed) < core_hi[k]))
            if r > 0:
                assert all(lab[s] == 7 for s in seeds)
        assert seen == sorted(set(seen)) and (r > 0 or seen == list(range(12)))
        assert r == 0 or sorted(len(seeds) for _, _, seeds in calls) == [6, 14, 16]
    # equal to the whole-volume statement: the same voxels summed in the same order
    want = whole_volume(lab, skels)
    for k in (7, 9):
        assert skels[k].cross_sectional_area.tobytes() == want[k][0].tobytes()
        assert np.array_equal(skels[k].cross_sectional_area_contacts, want[k][1])
    assert np.all(skels[7].cross_sectional_area == 144) and np.all(skels[9].cross_sectional_area == 16)
    for k in (5, 77):                                    # one voxel, none: skipped as cross_sectional_area skips them
        assert np.all(skels[k].cross_sectional_area == -1) and skels[k].cross_sectional_area.dtype == np.float32
        assert np.all(skels[k].cross_sectional_area_contacts == 0) and skels[k].cross_sectional_area_contacts.dtype == np.uint8
    for s in skels.values():
        ids = [a["id"] for a in s.extra_attributes]
        assert ids.count("cross_sectional_area") == 1 and ids.count("cross_sectional_area_contacts") == 1


def test_bit_64_when_the_growth_is_stopped():
    from kimimaro_amd import post
    lab, skels = bar_dataset()
    fake, timings = B.FakeSections(), {}
    largest = 20 * 18 * 18                               # of the round-0 boxes
    post.cross_sectional_area_chunked(lab, skels, chunk_shape=CHUNK, halo=2, max_box_voxels=largest, timings=timings, _sections=fake)
    # at halo 4 the boxes of the cores x < 32 hold 20^3 voxels or more and are not loaded; that of the last core, [28, 40) in x, is,
    # and its six sections stop at halo 8
    assert timings["calls"][0] == {"boxes": [12, 1, 0], "items": [42, 36, 6]} and timings["capped_items"] == 36
    assert np.all(skels[7].cross_sectional_area_contacts & 64)
    x = skels[7].vertices[:, 0]
    assert np.all(skels[7].cross_sectional_area[x < 32] == 12 * 8)      # y 10 .. 17 of the box [0, 18): the value of round 0
    assert np.all(skels[7].cross_sectional_area[x >= 32] == 12 * 10)    # y 10 .. 19 of the box [0, 20): the value of round 1
    want = whole_volume(lab, skels)
    assert np.array_equal(skels[7].cross_sectional_area_contacts & 63, want[7][1])
    assert skels[9].cross_sectional_area.tobytes() == want[9][0].tobytes()
    assert np.array_equal(skels[9].cross_sectional_area_contacts, want[9][1])
    with pytest.raises(ValueError):                      # a box of round 0 has to fit
        post.cross_sectional_area_chunked(lab, bar_dataset()[1], chunk_shape=CHUNK, halo=2, max_box_voxels=largest - 1, _sections=fake)


def test_arguments():
    from kimimaro_amd import post
    lab, skels = bar_dataset()
    for halo in (0, -3, 1.5):
        with pytest.raises(ValueError):
            post.cross_sectional_area_chunked(lab, skels, chunk_shape=CHUNK, halo=halo, _sections=B.FakeSections())
    with pytest.raises(NotImplementedError):
        post.cross_sectional_area_chunked(lab, skels, chunk_shape=CHUNK, halo=2, fill_holes=True, _sections=B.FakeSections())
    with pytest.raises(NotImplementedError):
        post.cross_sectional_area_chunked(lab, skels, chunk_shape=CHUNK, halo=2, visualize_section_planes=True, _sections=B.FakeSections())
    assert not hasattr(skels[7], "cross_sectional_area")


def test_exported():
    import kimimaro_amd
    from kimimaro_amd import post
    assert kimimaro_amd.cross_sectional_area_chunked is post.cross_sectional_area_chunked
