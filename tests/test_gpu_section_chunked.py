"""cross_sectional_area_chunked on the MI355X: kh_cross_sections_box against the CPU statement of the cropped box
(tests/section_box_ref.py) and, bit for bit, against kh_cross_sections on the whole volume; the driver against cross_sectional_area
on volumes that fit, and on a dataset of 2^32 voxels that cross_sectional_area refuses.

Against the statement: `voxels`, `contact` and `clip` equal, `area` within the 2 float32 ulps of tests/test_gpu_section.py.  Between
two device runs (box / whole volume, chunked / whole volume) areas are compared as bits: the same voxels are summed as integers of
the same fixed point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chunked_ref as R  # noqa: E402
import section_box_ref as B  # noqa: E402
from shapes import random_walk_tube, voronoi_labels  # noqa: E402

pytestmark = pytest.mark.gpu

ANISOTROPIES = [(1, 1, 1), (4, 4, 40)]
CHUNK, HALO = (16, 16, 16), 4
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def tube():
    return cached("tube", lambda: random_walk_tube((64, 56, 48), 5, steps=60))


def items():
    """80 foreground seeds of the tube and their normals, from one generator"""
    def make():
        rng = np.random.default_rng(3)
        where = np.argwhere(tube() != 0)
        return where[rng.integers(0, len(where), size=80)], rng.normal(size=(80, 3))
    return cached("items", make)


def within_ulps(got, want64, ulps=2):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)


def device_whole(labels, seeds, normals, wants, anisotropy):
    from kimimaro_amd import ops, section, utility
    eng = ops.engine()
    d_flat, itemsize, _, shape, _, span = utility._device_labels(eng, labels)
    d_lab, label_bytes, word = utility._narrow_labels(eng, d_flat, itemsize, span, set(int(w) for w in wants))
    words = np.array([word[int(w)] for w in wants], dtype=np.uint32)
    return section.cross_sections(eng, d_lab, label_bytes, shape, anisotropy, section.seed_index(seeds, shape), words, normals)


def device_boxes(labels, seeds, normals, wants, anisotropy, chunk=CHUNK, halo=HALO):
    """every item in the box of its core, one kh_cross_sections_box launch per box -> (area, contact, clip, voxels, boxes [n, 2, 3])"""
    from kimimaro_amd import ops, section, utility
    eng = ops.engine()
    n = len(seeds)
    out = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    boxes = np.array([B.halo_box(s, chunk, halo, labels.shape) for s in seeds])
    for lo, hi in sorted({(tuple(b[0]), tuple(b[1])) for b in boxes.tolist()}):
        sel = np.flatnonzero(np.all(boxes[:, 0] == lo, axis=1) & np.all(boxes[:, 1] == hi, axis=1))
        crop = np.asfortranarray(labels[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
        d_flat, itemsize, _, shape, _, span = utility._device_labels(eng, crop)
        d_lab, label_bytes, word = utility._narrow_labels(eng, d_flat, itemsize, span, set(int(w) for w in wants))
        words = np.array([word[int(wants[i])] for i in sel], dtype=np.uint32)
        got = section.cross_sections_box(eng, d_lab, label_bytes, lo, shape, labels.shape, anisotropy,
                                         section.seed_index(seeds[sel] - np.array(lo), shape), words, normals[sel])
        for a, g in zip(out, got):
            a[sel] = g
    return out + (boxes,)


# ---- 1. the kernel against the statement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anisotropy", ANISOTROPIES)
def test_box_kernel_against_the_statement(anisotropy):
    labels = tube()
    seeds, normals = items()
    area, contact, clip, voxels, boxes = device_boxes(labels, seeds, normals, np.ones(80, dtype=int), anisotropy)
    want = []
    for seed, n, (lo, hi) in zip(seeds, normals, boxes):
        crop = labels[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        want.append(B.section_in_box(crop, lo, labels.shape, tuple(seed - lo), n, anisotropy, 1))
    clipped = sum(1 for w in want if w[3] != 0)
    print("clipped in the statement: %d of 80" % clipped)
    assert clipped >= 10 and 80 - clipped >= 10
    assert clipped == (39 if anisotropy == (1, 1, 1) else 38)
    for k, w in enumerate(want):
        print("item %d: voxels %d / %d, contact %d / %d, clip %d / %d, area %r / %r" % (k, voxels[k], w[0], contact[k], w[2], clip[k], w[3],
                                                                                     area[k], w[1]))
        assert int(voxels[k]) == w[0] and int(contact[k]) == w[2] and int(clip[k]) == w[3], k
        assert within_ulps(area[k], w[1]), (k, area[k], w[1])


# ---- 2. box against whole, bit for bit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anisotropy", ANISOTROPIES)
def test_box_equals_whole_volume_where_nothing_is_clipped(anisotropy):
    labels = tube()
    seeds, normals = items()
    wants = np.ones(80, dtype=int)
    w_area, w_contact, w_voxels = device_whole(labels, seeds, normals, wants, anisotropy)
    area, contact, clip, voxels, _ = device_boxes(labels, seeds, normals, wants, anisotropy)
    free = clip == 0
    assert free.sum() >= 10 and (~free).sum() >= 10
    assert np.array_equal(voxels[free], w_voxels[free]) and np.array_equal(contact[free], w_contact[free])
    assert area[free].tobytes() == w_area[free].tobytes()
    assert np.all(voxels[~free] <= w_voxels[~free]) and np.all(voxels[~free] > 0)
    # the box that is the whole volume
    area, contact, clip, voxels, boxes = device_boxes(labels, seeds, normals, wants, anisotropy, chunk=labels.shape, halo=1)
    assert np.all(boxes[:, 0] == 0) and np.all(boxes[:, 1] == labels.shape)
    assert np.all(clip == 0) and np.array_equal(voxels, w_voxels) and np.array_equal(contact, w_contact)
    assert area.tobytes() == w_area.tobytes()


# ---- 3. the driver against the whole-volume function ----------------------------------------------------------------------------------

def driver_case(volume, anisotropy):
    """(labels, {label: Skeleton} from skeletonize)"""
    def make():
        import kimimaro_amd
        labels = tube() if volume == "tube" else voronoi_labels((48, 44, 40), 10, 8, anisotropy=anisotropy)
        skels = kimimaro_amd.skeletonize(labels, anisotropy=anisotropy, dust_threshold=100, progress=False)
        assert len(skels) >= (1 if volume == "tube" else 8)
        return labels, skels
    return cached((volume, anisotropy), make)


def fresh(skels, shift=(0, 0, 0), anisotropy=(1, 1, 1), ids=None):
    from kimimaro_amd import Skeleton
    move = (np.array(shift, dtype=np.float32) * np.array(anisotropy, dtype=np.float32))
    return {k: Skeleton(s.vertices + move, s.edges.copy(), segid=k if ids is None else ids[k], space="physical") for k, s in skels.items()}


def whole_run(volume, anisotropy, smoothing_window, step):
    def make():
        import kimimaro_amd
        labels, skels = driver_case(volume, anisotropy)
        return kimimaro_amd.cross_sectional_area(labels, fresh(skels), anisotropy, smoothing_window, step=step)
    return cached((volume, anisotropy, smoothing_window, step, "whole"), make)


def assert_same_sections(got, want):
    assert list(got) == list(want)
    for k in want:
        a, b = got[k], want[k]
        assert a.cross_sectional_area.dtype == np.float32 and a.cross_sectional_area_contacts.dtype == np.uint8
        assert a.cross_sectional_area.tobytes() == b.cross_sectional_area.tobytes(), k
        assert np.array_equal(a.cross_sectional_area_contacts, b.cross_sectional_area_contacts), k
        ids = [p["id"] for p in a.extra_attributes]
        assert ids.count("cross_sectional_area") == 1 and ids.count("cross_sectional_area_contacts") == 1


@pytest.mark.parametrize("volume", ["tube", "voronoi"])
@pytest.mark.parametrize("anisotropy", ANISOTROPIES)
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("smoothing_window", [1, 5])
def test_driver_equals_cross_sectional_area(smoothing_window, step, anisotropy, volume):
    import kimimaro_amd
    labels, skels = driver_case(volume, anisotropy)
    want = whole_run(volume, anisotropy, smoothing_window, step)
    mine, timings = fresh(skels), {}
    out = kimimaro_amd.cross_sectional_area_chunked(labels, mine, chunk_shape=CHUNK, halo=HALO, anisotropy=anisotropy,
                                                    smoothing_window=smoothing_window, step=step, timings=timings)
    print(timings)
    assert out is mine
    assert_same_sections(mine, want)
    assert sum(int((s.cross_sectional_area > 0).sum()) for s in mine.values()) > 0
    assert not any(np.any(s.cross_sectional_area_contacts & 64) for s in mine.values()) and timings["capped_items"] == 0
    cores = int(np.prod([-(-n // c) for n, c in zip(labels.shape, CHUNK)]))
    first = timings["calls"][0]
    assert timings["cores"] == cores and first["boxes"][0] == cores               # round 0 loaded every core exactly once ...
    assert all(call["boxes"][0] <= cores for call in timings["calls"])
    assert len(first["boxes"]) >= 2 and first["boxes"][1] >= 1 and first["items"][1] >= 1 and timings["items_rerun"] >= 1     # ... and a growth round ran
    assert timings["kernel_ms"] > 0 and timings["voxels_loaded"] >= labels.size


# ---- 4. a dataset cross_sectional_area cannot take ------------------------------------------------------------------------------------

class Corner:
    """2048 x 2048 x 1024 voxels, zero but for one small volume at `lo`; boxes away from it are served from shared zero arrays"""
    shape = (2048, 2048, 1024)

    def __init__(self, small, lo):
        self.small, self.lo, self.zeros = small, np.array(lo), {}

    def __getitem__(self, key):
        lo = np.array([s.start for s in key])
        hi = np.array([s.stop for s in key])
        ext = tuple(int(v) for v in hi - lo)
        a, b = np.maximum(lo, self.lo), np.minimum(hi, self.lo + self.small.shape)
        if np.any(a >= b):
            if ext not in self.zeros:
                self.zeros[ext] = np.zeros(ext, dtype=self.small.dtype, order="F")
            return self.zeros[ext]
        out = np.zeros(ext, dtype=self.small.dtype, order="F")
        out[tuple(slice(int(p - o), int(q - o)) for p, q, o in zip(a, b, lo))] = \
            self.small[tuple(slice(int(p - o), int(q - o)) for p, q, o in zip(a, b, self.lo))]
        return out


def test_dataset_of_2_to_the_32_voxels():
    import kimimaro_amd
    labels, skels = driver_case("tube", (1, 1, 1))
    want = whole_run("tube", (1, 1, 1), 1, 1)
    lo = (1529, 1516, 483)                               # across the cuts at 1536, 1536 and 512, where sections reach 8 voxels past them
    dataset = Corner(labels, lo)
    assert np.prod(dataset.shape, dtype=np.int64) == 2 ** 32
    with pytest.raises(ValueError):
        kimimaro_amd.cross_sectional_area(np.broadcast_to(np.zeros(1, dtype=np.uint8), dataset.shape), fresh(skels, lo))
    mine, timings = fresh(skels, lo), {}
    kimimaro_amd.cross_sectional_area_chunked(dataset, mine, chunk_shape=(512, 512, 512), halo=8, timings=timings)
    print(timings)
    assert timings["cores"] == 32 and timings["calls"][0]["boxes"][0] == 32 and timings["voxels_loaded"] >= 2 ** 32
    assert timings["items_rerun"] >= 1 and timings["capped_items"] == 0
    for k in want:
        # outside the small volume there is background: the same voxels, but no face of the dataset is near
        assert mine[k].cross_sectional_area.tobytes() == want[k].cross_sectional_area.tobytes()
        assert np.all(mine[k].cross_sectional_area_contacts == 0)
        assert np.any(want[k].cross_sectional_area_contacts == 0) and np.any(mine[k].cross_sectional_area > 0)


# ---- 5. bit 64 ----------------------------------------------------------------------------------------------------------------------

def test_bit_64_marks_what_stayed_clipped():
    """chunks of (32, 28, 24): eight cores, every box of round 0 holds 36 * 32 * 28 voxels and every box at halo 8 more"""
    import kimimaro_amd
    from kimimaro_amd import utility
    labels, skels = driver_case("tube", (1, 1, 1))
    want = whole_run("tube", (1, 1, 1), 1, 1)
    chunk, timings = (32, 28, 24), {}
    mine = fresh(skels)
    kimimaro_amd.cross_sectional_area_chunked(labels, mine, chunk_shape=chunk, halo=4, max_box_voxels=36 * 32 * 28, timings=timings)
    print(timings)
    assert all(call["boxes"][1:] == [0] * (len(call["boxes"]) - 1) for call in timings["calls"]) and timings["capped_items"] >= 1
    marked = 0
    for k, s in mine.items():
        # round 0 of every vertex that is evaluated once: its first occurrence in the box of its core
        vox, occ_vertex, occ_normal = utility._xs_occurrences(s, np.ones(3, dtype=np.float32), (0, 0, 0), labels.shape, 1, 1)
        vertex, first = np.unique(occ_vertex, return_index=True)
        once = ~np.isin(vertex, s.branches())
        vertex, first = vertex[once], first[once]
        area, contact, clip, voxels, _ = device_boxes(labels, vox[vertex], occ_normal[first], np.full(len(vertex), k), (1, 1, 1), chunk, 4)
        assert np.all(area > 0)
        hit = clip != 0
        assert np.array_equal((s.cross_sectional_area_contacts[vertex] & 64) != 0, hit)
        assert s.cross_sectional_area[vertex[hit]].tobytes() == area[hit].tobytes()
        assert np.array_equal(s.cross_sectional_area_contacts[vertex[hit]], contact[hit] | 64)
        keep = vertex[~hit]
        assert s.cross_sectional_area[keep].tobytes() == want[k].cross_sectional_area[keep].tobytes()
        assert np.array_equal(s.cross_sectional_area_contacts[keep], want[k].cross_sectional_area_contacts[keep])
        marked += int(hit.sum())
    assert marked >= 1


# ---- 6. the keyword of skeletonize_chunked --------------------------------------------------------------------------------------------

def test_keyword_of_skeletonize_chunked():
    import kimimaro_amd
    kw = dict(teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST, post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK,
              width=2)
    xs = dict(chunk_shape=(32, 32, 32), halo=8, smoothing_window=3)
    both = kimimaro_amd.skeletonize_chunked(R.dataset(0), R.DATASETS[0][3], cross_sectional_area=xs, **kw)
    plain = kimimaro_amd.skeletonize_chunked(R.dataset(0), R.DATASETS[0][3], **kw)
    assert len(plain) >= 8
    assert not any(hasattr(s, "cross_sectional_area") or hasattr(s, "cross_sectional_area_contacts") for s in plain.values())
    R.assert_same(both, plain)
    after = kimimaro_amd.cross_sectional_area_chunked(R.dataset(0), plain, anisotropy=R.AN, **xs)
    assert_same_sections(both, after)
    assert any(np.any(s.cross_sectional_area > 0) for s in both.values())


# ---- 7. labels and skips --------------------------------------------------------------------------------------------------------------

def test_uint64_labels_and_an_absent_label():
    import kimimaro_amd
    from kimimaro_amd import Skeleton
    labels, skels = driver_case("voronoi", (1, 1, 1))
    want = whole_run("voronoi", (1, 1, 1), 1, 1)
    big = np.asfortranarray(labels.astype(np.uint64) + np.uint64(2 ** 40))
    big[0, 0, 0] = 55555                                 # a label of one voxel
    ids = {k: int(k) + 2 ** 40 for k in skels}
    mine = fresh(skels, ids=ids)
    first = next(iter(mine))
    corner = int(labels[0, 0, 0])                        # (its label loses that voxel: left out of the comparison)
    extra = [Skeleton(mine[first].vertices.copy(), mine[first].edges.copy(), segid=77777, space="physical"),
             Skeleton(mine[first].vertices.copy(), mine[first].edges.copy(), segid=0, space="physical"),
             Skeleton(np.array([[0, 0, 0], [1, 0, 0]]), np.array([[0, 1]]), segid=55555, space="physical")]
    arg = extra + [s for k, s in mine.items() if k != corner]
    out = kimimaro_amd.cross_sectional_area_chunked(big, arg, chunk_shape=CHUNK, halo=HALO)
    assert out is arg
    for s in extra:
        assert s.cross_sectional_area.dtype == np.float32 and np.all(s.cross_sectional_area == -1)
        assert s.cross_sectional_area_contacts.dtype == np.uint8 and np.all(s.cross_sectional_area_contacts == 0)
        assert len(s.cross_sectional_area) == len(s.vertices)
        assert [a["id"] for a in s.extra_attributes].count("cross_sectional_area") == 1
    assert_same_sections({k: s for k, s in mine.items() if k != corner}, {k: s for k, s in want.items() if k != corner})


def test_bool_volume():
    import kimimaro_amd
    labels, skels = driver_case("voronoi", (1, 1, 1))
    first = next(iter(skels))
    mask = np.asfortranarray(labels == first)
    a = fresh({first: skels[first]}, ids={first: 424242})[first]       # a bool volume gives every skeleton label 1
    b = fresh({first: skels[first]}, ids={first: 424242})[first]
    kimimaro_amd.cross_sectional_area(mask, a)
    kimimaro_amd.cross_sectional_area_chunked(mask, b, chunk_shape=CHUNK, halo=HALO)
    assert_same_sections({first: b}, {first: a})
    assert np.any(b.cross_sectional_area > 0)
