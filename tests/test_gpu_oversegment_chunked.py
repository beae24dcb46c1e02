"""oversegment_chunked on the MI355X: the three kernels of a dataset in boxes against numpy -- kh_box_shell_diff,
kh_first_appearance_box (past 2^32 too), kh_geodesic_seed_at --, then the driver against kimimaro_amd.oversegment of the same array on
the same device: features, dtype, segments, and the distance store bit for bit against the d_dist of feature.geodesic_voronoi."""
import numpy as np
import pytest

import feature_ref as R
import oversegment_chunked_ref as H

pytestmark = pytest.mark.gpu

BOXES = [(5, 4, 3), (70, 9, 6), (66, 6, 6)]


def engine():
    from kimimaro_amd import ops
    return ops.engine()


def cores_of(box):
    """cores that touch 0, 1 and 3 faces of the box (no halo on those sides); (66, 6, 6): the core [1, 65) in x"""
    b = np.array(box)
    return [(np.array([1, 1, 1]), b - 1), (np.array([0, 1, 1]), b - 1), (np.array([0, 0, 0]), b - 1)]


def up(eng, a):
    """a host box [x, y, z] of 32-bit words -> device, Fortran order"""
    import torch
    flat = np.asfortranarray(a).reshape(-1, order="F")
    return torch.from_numpy(flat.view(np.int32) if flat.dtype != np.float32 else flat).to(eng.device)


def diff(eng, old, now, lo, hi):
    from kimimaro_amd import feature
    return feature.box_shell_diff(eng, up(eng, old), up(eng, now), old.shape, lo, hi)


# ---- kh_box_shell_diff ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES)
def test_shell_diff_single_voxels(box):
    """one changed voxel at each of the 26 shell positions, in the interior, in the halo -> the bits numpy names; where the core is
    three voxels thick or more on every axis, exactly the directions that agree with the position on its non-zero axes"""
    from kimimaro_amd import post
    eng = engine()
    rng = np.random.default_rng(3)
    old = rng.integers(0, 2 ** 31, size=box, dtype=np.uint32)
    for lo, hi in cores_of(box):
        n = hi - lo
        mid = lo + n // 2
        for k, step in enumerate(R.directions()):
            at = tuple(int(l if d < 0 else h - 1 if d > 0 else m) for d, l, h, m in zip(step, lo, hi, mid))
            now = old.copy()
            now[at] ^= 1
            got = diff(eng, old, now, lo, hi)
            assert got == post.shell_diff(old, now, lo, hi), (box, lo, hi, step)
            assert got[1] == 1 and (got[0] >> k) & 1
            if np.all(n >= 3):
                want = sum(1 << j for j, other in enumerate(R.directions()) if all(o == 0 or o == d for o, d in zip(other, step)))
                assert got[0] == want, (box, lo, hi, step)
        if np.all(n >= 3):
            now = old.copy()
            now[tuple(int(v) for v in mid)] ^= 1
            assert diff(eng, old, now, lo, hi)[:2] == (0, 1)              # an interior voxel: nobody has to look again
        outside = [a for a in range(3) if lo[a] > 0]
        if outside:
            now = old.copy()
            at = [int(v) for v in mid]
            at[outside[0]] = 0
            now[tuple(at)] ^= 1
            assert diff(eng, old, now, lo, hi)[:2] == (0, 0)              # a halo voxel: nothing


@pytest.mark.parametrize("box", BOXES)
def test_shell_diff_random_changes(box):
    """distances with infinities, a negative value and NaN among them: mask, count and the largest finite value"""
    from kimimaro_amd import post
    eng = engine()
    rng = np.random.default_rng(4)
    for trial, (lo, hi) in enumerate(cores_of(box)):
        old = (rng.random(box) * 1000).astype(np.float32)
        old[rng.random(box) < 0.3] = np.inf
        now = old.copy()
        hit = rng.random(box) < (0.02, 0.3, 0.0)[trial]
        now[hit] = (rng.random(int(hit.sum())) * 500).astype(np.float32)
        if trial == 1:
            now[tuple(int(v) for v in lo)] = np.float32(-3.0)
            now[tuple(int(v) for v in hi - 1)] = np.float32(np.nan)
        got = diff(eng, old, now, lo, hi)
        want = post.shell_diff(old, now, lo, hi)
        assert got == want
        core = now[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))]
        finite = core[np.isfinite(core) & (core >= 0)]
        assert np.uint32(got[2]).view(np.float32) == (finite.max() if finite.size else 0)
        if trial == 2:
            assert got[:2] == (0, 0)
    all_inf = np.full(box, np.inf, dtype=np.float32)
    assert diff(eng, all_inf, all_inf, (0, 0, 0), box) == (0, 0, 0)


# ---- kh_first_appearance_box -----------------------------------------------------------------------------------------------------
def first_appearance_host(f, lo, hi, origin, SX, SY, nnumbers, first):
    for x in range(lo[0], hi[0]):
        for y in range(lo[1], hi[1]):
            for z in range(lo[2], hi[2]):
                n = int(f[x, y, z])
                if 0 < n <= nnumbers:
                    index = (origin[0] + x) + SX * ((origin[1] + y) + SY * (origin[2] + z))
                    first[n] = index if first[n] < 0 else min(first[n], index)


def runs_of_numbers(rng, box, nnumbers):
    """numbers in runs along x (the kernel spends one atomic per run), 0, numbers above nnumbers and the "none" word among them"""
    f = rng.integers(0, nnumbers + 3, size=box, dtype=np.uint32)
    f = np.repeat(f[::3], 3, axis=0)[:box[0]]
    f[rng.random(box) < 0.1] = 0
    f[rng.random(box) < 0.1] = H.NONE
    return np.asfortranarray(f)


@pytest.mark.parametrize("box", BOXES)
def test_first_appearance_box(box):
    from kimimaro_amd import feature
    eng = engine()
    rng = np.random.default_rng(5)
    nn = 40
    for lo, hi in cores_of(box):
        f = runs_of_numbers(rng, box, nn)
        # origin 0 in a dataset of the box's size, and a virtual dataset whose indices pass 2^32: only the box exists
        for origin, SX, SY in (((0, 0, 0), box[0], box[1]), ((2900, 2950, 590), 3000, 3000)):
            d_first = feature.first_appearance_table(eng, nn)
            feature.first_appearance_box(eng, up(eng, f), box, lo, hi, origin, SX, SY, nn, d_first)
            want = np.full(nn + 1, -1, dtype=np.int64)
            first_appearance_host(f, lo, hi, origin, SX, SY, nn, want)
            np.testing.assert_array_equal(d_first.cpu().numpy(), want)
            assert want[0] == -1 and (want.max() >= 2 ** 32) == (SX == 3000)


def test_first_appearance_accumulates_over_boxes():
    from kimimaro_amd import feature
    eng = engine()
    rng = np.random.default_rng(6)
    box, nn = (70, 9, 6), 25
    a, b = runs_of_numbers(rng, box, nn), runs_of_numbers(rng, box, nn)
    lo, hi = (1, 0, 0), (69, 9, 6)
    d_first = feature.first_appearance_table(eng, nn)
    want = np.full(nn + 1, -1, dtype=np.int64)
    for f, origin in ((b, (69, 0, 0)), (a, (0, 0, 0))):                  # (in the opposite order of the raster)
        feature.first_appearance_box(eng, up(eng, f), box, lo, hi, origin, 140, 9, nn, d_first)
        first_appearance_host(f, lo, hi, origin, 140, 9, nn, want)
    np.testing.assert_array_equal(d_first.cpu().numpy(), want)
    lut, K = feature.first_appearance_map(want)
    owned = np.flatnonzero(want[1:] >= 0) + 1
    assert K == owned.size and sorted(lut[owned].tolist()) == list(range(1, K + 1))
    assert np.all(np.diff(want[owned][np.argsort(lut[owned])]) > 0)


# ---- kh_geodesic_seed_at -----------------------------------------------------------------------------------------------------------
def test_seed_at_touches_the_seeds_only():
    from kimimaro_amd import feature
    eng = engine()
    rng = np.random.default_rng(7)
    box = (70, 9, 6)
    nvox = 70 * 9 * 6
    lab = rng.integers(0, 3, size=nvox).astype(np.uint16)
    d0 = (rng.random(nvox) * 100).astype(np.float32)
    f0 = rng.integers(50, 90, size=nvox, dtype=np.uint32)
    on1 = np.flatnonzero(lab == 1)
    voxel = np.array([on1[0], on1[5], on1[5], on1[9], np.flatnonzero(lab == 2)[0], np.flatnonzero(lab == 0)[0]], dtype=np.uint32)
    number = np.array([7, 30, 12, 99, 3, 4], dtype=np.uint32)            # a shared voxel: 12 wins; 99 loses to what is there
    label = np.array([1, 1, 1, 1, 1, 1], dtype=np.uint32)                # the last two sit off label 1
    d_lab = eng.to_device(lab)
    want_d, want_f = d0.copy(), f0.copy()
    want_d[voxel[:4]] = 0
    want_f[on1[0]], want_f[on1[5]], want_f[on1[9]] = 7, 12, min(99, int(f0[on1[9]]))
    d_d, d_f = up(eng, d0), up(eng, f0)
    feature.seed_at(eng, d_lab, 2, nvox, voxel, number, label, d_dist=d_d, d_feat=d_f)
    np.testing.assert_array_equal(d_d.cpu().numpy(), want_d)
    np.testing.assert_array_equal(d_f.cpu().numpy().view(np.uint32), want_f)
    # one array alone: the other is left out
    d_d, d_f = up(eng, d0), up(eng, f0)
    feature.seed_at(eng, d_lab, 2, nvox, voxel, number, label, d_dist=d_d)
    feature.seed_at(eng, d_lab, 2, nvox, voxel, number, label, d_feat=d_f)
    np.testing.assert_array_equal(d_d.cpu().numpy(), want_d)
    np.testing.assert_array_equal(d_f.cpu().numpy().view(np.uint32), want_f)
    assert box[0] * box[1] * box[2] == nvox


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def whole(lab, skels, an):
    """kimimaro_amd.oversegment of the whole array and the distances its geodesic_voronoi call left on the device"""
    import kimimaro_amd
    from kimimaro_amd import feature
    kept, real = {}, feature.geodesic_voronoi

    def spy(*args, **kw):
        out = real(*args, **kw)
        kept["d"] = out[0].cpu().numpy()
        return out

    feature.geodesic_voronoi = spy
    try:
        f, s = kimimaro_amd.oversegment(lab, skels, anisotropy=an)
    finally:
        feature.geodesic_voronoi = real
    return f, s, kept["d"]


def assert_same(lab, skels, an, chunk, dataset=None, **kw):
    import kimimaro_amd
    shape = (tuple(lab.shape) + (1,))[:3]
    store = np.full(shape, -1.0, dtype=np.float32, order="F")
    timings = {}
    got_f, got_s = kimimaro_amd.oversegment_chunked(lab if dataset is None else dataset, skels, chunk_shape=chunk, anisotropy=an,
                                                    distance_store=store, timings=timings, **kw)
    want_f, want_s, want_d = whole(lab, skels, an)
    assert got_f.dtype == want_f.dtype and got_f.shape == want_f.shape
    np.testing.assert_array_equal(got_f, want_f)
    H.assert_skeletons(got_s, want_s, skels)
    np.testing.assert_array_equal(store.reshape(-1, order="F").view(np.uint32), want_d.view(np.uint32))
    assert timings["segments"] == int(want_f.max())
    return got_f, got_s, timings


@pytest.mark.parametrize("an", [(16, 16, 40), (1, 1, 1)])
def test_random_volume(an):
    lab, skels = H.random_blobs(np.random.default_rng(21), (45, 23, 17), nlabels=5, nseeds=24, an=an)
    got_f, _, timings = assert_same(lab, skels, an, (16, 8, 8))
    assert timings["cores"] == 3 * 3 * 3 and got_f.max() > 5


@pytest.mark.parametrize("chunk", [(64, 4, 4), (65, 4, 4)])
def test_wider_than_a_wave_and_a_brick(chunk):
    lab, skels = H.random_blobs(np.random.default_rng(22), (70, 9, 6), nlabels=3, nseeds=12)
    assert_same(lab, skels, (4, 4, 40), chunk)


@pytest.mark.parametrize("rows,sx,chunk", [(6, 16, (8, 64, 1)), (5, 130, (64, 64, 1))])
def test_serpentine(rows, sx, chunk):
    lab = H.serpentine(rows, sx)
    got_f, _, timings = assert_same(lab, H.skel(7, [[0, 0, 0]]), (1, 1, 1), chunk)
    assert np.all(got_f[lab != 0] == 1) and timings["distance_visits"] >= rows and timings["feature_visits"] >= rows


@pytest.mark.parametrize("name,build", H.CASES, ids=[c[0] for c in H.CASES])
def test_shared_cases(name, build):
    """the host file's cases: skip rules, ties on a cut plane, a grid edge and a grid corner, the U-turn, the numbering, uint64 labels,
    a bool dataset, two axes, one box"""
    lab, skels, an, chunk = build()
    assert_same(lab, skels, an, chunk)


def test_uint16_result():
    lab, s = H.long_line()
    got_f, _, _ = assert_same(lab, s, (1, 1, 1), (64, 2, 2))
    assert got_f.dtype == np.uint16 and got_f.max() == 300


def test_device_tensor_dataset_and_a_feature_store():
    import torch
    import kimimaro_amd
    lab, skels = H.skip_volume()
    assert_same(lab, skels, (1, 1, 1), (6, 5, 4), dataset=torch.from_numpy(lab.astype(np.int32)).to("cuda"))
    store = np.zeros(lab.shape, dtype=np.uint32, order="F")
    got_f, _ = kimimaro_amd.oversegment_chunked(lab, skels, chunk_shape=(6, 5, 4), feature_store=store)
    want_f, _ = kimimaro_amd.oversegment(lab, skels)
    assert got_f is store
    np.testing.assert_array_equal(store, want_f)


def test_composes_with_skeletonize_chunked():
    """the skeletons skeletonize_chunked has just made of the dataset, in its own chunks: dict in -> dict out"""
    import kimimaro_amd
    from shapes import voronoi_labels
    an = (16, 16, 40)
    lab = voronoi_labels((64, 64, 48), 10, seed=5, pts_per_label=5, step=10.0, anisotropy=an)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 64
    skels = kimimaro_amd.skeletonize_chunked(lab, (32, 32, 32), teasar_params=params, anisotropy=an, dust_threshold=200,
                                             post_dust_threshold=0.0, tick_threshold=0.0, width=2)
    assert len(skels) > 0
    got_f, got_s, timings = assert_same(lab, skels, an, (32, 32, 32))
    assert timings["cores"] == 8 and got_f.max() > len(skels)
    assert all((s.segments != 0).all() for s in got_s.values())


def test_host_seam_visits_the_same_cores():
    """the visiting order is raster order both ways, so the counts of the seam and of the kernels are the same numbers"""
    import kimimaro_amd
    lab, skels = H.random_blobs(np.random.default_rng(1003), (17, 8, 9), an=(1.5, 1, 3))
    on_device, on_host = {}, {}
    got = kimimaro_amd.oversegment_chunked(lab, skels, chunk_shape=(6, 3, 4), anisotropy=(1.5, 1, 3), timings=on_device)
    want = kimimaro_amd.oversegment_chunked(lab, skels, chunk_shape=(6, 3, 4), anisotropy=(1.5, 1, 3), timings=on_host, _box=H.relax_box)
    np.testing.assert_array_equal(got[0], want[0])
    for key in ("distance_visits", "feature_visits", "distance_rounds", "feature_rounds", "boxes_loaded", "voxels_loaded", "segments"):
        assert on_device[key] == on_host[key], key
