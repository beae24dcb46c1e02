"""GPU: kimimaro_amd.oversegment (csrc/feature.hip) == the CPU statement of its contract (tests/feature_ref.py) -- every voxel of
the label volume and every entry of every `segments` array, exactly; for the function-level mirror
ops.euclidean_distance_field(..., return_feature_map=True) also the field, bit for bit."""
import numpy as np
import pytest

import feature_ref as R
from shapes import random_walk_tube, voronoi_labels
from test_oversegment_host import skeletons_for, two_label_volume

pytestmark = pytest.mark.gpu

ANISOTROPIES = [(1, 1, 1), (16, 16, 40), (0.5, 1.25, 3.0)]


def assert_same(lab, skels, an):
    import kimimaro_amd
    stats = {}
    got_f, got_s = kimimaro_amd.oversegment(lab, skels, anisotropy=an, _stats=stats)
    want_f, want_s, _ = R.oversegment(lab, skels, an)
    assert got_f.dtype == want_f.dtype and got_f.shape == want_f.shape
    np.testing.assert_array_equal(got_f, want_f)
    assert type(got_s) is type(want_s)
    if isinstance(skels, dict):
        assert list(got_s) == list(want_s)
    for g, w, original in zip(R.skeleton_list(got_s), R.skeleton_list(want_s), R.skeleton_list(skels)):
        assert g is not original and not hasattr(original, "segments")
        assert g.segments.dtype == np.uint64 and g.segments.shape == (len(g.vertices),)
        np.testing.assert_array_equal(g.segments, w.segments)
        np.testing.assert_array_equal(g.vertices, original.vertices)
        assert [a["id"] for a in g.extra_attributes].count("segments") == 1
        assert [a for a in g.extra_attributes if a["id"] == "segments"][0] == {"id": "segments", "data_type": "uint64", "num_components": 1}
    return got_f, got_s, stats


def skeletonize(lab, an, const):
    import kimimaro_amd
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = const
    skels = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=200, fix_borders=True, progress=False)
    assert len(skels) > 0
    return skels


# sides that are no multiples of the bricks (64 x 4 x 4) or of 64, more than one brick along every axis
@pytest.mark.parametrize("shape,an,const", [((64, 64, 48), (16, 16, 40), 64), ((83, 45, 33), (1, 1, 1), 4),
                                            ((70, 41, 30), (0.5, 1.25, 3.0), 4)])
def test_composes_with_skeletonize(shape, an, const):
    """the skeletons skeletonize() has just made of a dense tessellation (the volume of smoke()), dict in -> dict out"""
    lab = voronoi_labels(shape, 10, seed=5, pts_per_label=5, step=10.0, anisotropy=an)
    skels = skeletonize(lab, an, const)
    got_f, got_s, stats = assert_same(lab, skels, an)
    assert got_f.max() > len(skels)                   # more segments than labels: the labels were cut
    assert all((s.segments != 0).all() for s in got_s.values())
    # list in -> list out, one -> one; the numbering follows the container's order
    assert_same(lab, list(skels.values())[::-1], an)
    one = next(iter(skels.values()))
    got_f1, got_s1, _ = assert_same(lab, one, an)
    assert hasattr(got_s1, "vertices") and set(np.unique(got_f1[lab != one.id])) == {0}


@pytest.mark.parametrize("an", ANISOTROPIES)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64, np.int32])
def test_awkward_skeletons(an, dtype):
    """a label with no skeleton, a skeleton whose label is absent, id 0, a one-voxel label, two vertices on one voxel, a vertex off
    its label, a vertex outside the volume, a label with two components of which one holds no vertex"""
    lab = two_label_volume().astype(dtype)
    got_f, got_s, _ = assert_same(lab, skeletons_for(an), an)
    assert got_f.max() == 6 and got_f.dtype == np.uint8
    assert got_s[5].segments[0] == 0 and got_s[9].segments[2] == 0


def test_wide_labels_and_a_lonely_component():
    """uint64 labels beyond 2^32 (renumbered on the device); a vertex on a one-voxel COMPONENT of a label that has other voxels is a
    seed (only a one-voxel LABEL is skipped)"""
    lab = np.zeros((12, 9, 6), dtype=np.uint64, order="F")
    lab[:6, :4] = 2 ** 40 + 5
    lab[6:, :4] = 2 ** 63 + 7
    lab[3, 7, 3] = 2 ** 40 + 5              # lonely voxel of the first label
    lab[9, 7, 3] = 77                       # a one-voxel label
    import kimimaro_amd
    S = kimimaro_amd.Skeleton
    skels = [S([[9, 1, 1], [7, 2, 4]], segid=2 ** 63 + 7), S([[4, 1, 1], [1, 1, 1], [3, 7, 3]], segid=2 ** 40 + 5),
             S([[9, 7, 3]], segid=77), S([[1, 1, 1]], segid=2 ** 40 + 6)]
    got_f, got_s, _ = assert_same(lab, skels, (1, 1, 1))
    assert got_f[3, 7, 3] != 0 and got_f[9, 7, 3] == 0 and got_f.max() == 5


def test_bool_volume():
    """every skeleton segments label 1 of a bool volume, whatever its id (kimimaro/utility.py:134-135)"""
    import kimimaro_amd
    mask = random_walk_tube((56, 50, 44), seed=11).astype(bool)
    pts = np.argwhere(mask)
    a = kimimaro_amd.Skeleton(pts[::701].astype(np.float32), segid=0)
    b = kimimaro_amd.Skeleton(pts[350::977].astype(np.float32), segid=12345)
    got_f, _, _ = assert_same(mask, {3: a, 4: b}, (1, 1, 1))
    assert got_f.max() > 1 and np.all(got_f[~mask] == 0)


def snake(shape=(150, 48, 90)):
    """a one-voxel-thick path of more than 200 voxels whose diagonal runs step through brick corners"""
    lab = np.zeros(shape, dtype=np.uint16, order="F")
    p = np.array([2, 2, 2])
    path = [tuple(p)]
    for step, n in (((1, 1, 1), 40), ((1, 0, 0), 60), ((1, -1, 1), 38), ((0, 1, -1), 40), ((-1, 0, -1), 30)):
        for _ in range(n):
            p = p + np.array(step)
            path.append(tuple(int(v) for v in p))
    for q in path:
        lab[q] = 300
    return lab, path


@pytest.mark.parametrize("an", [(1, 1, 1), (0.5, 1.25, 3.0)])
def test_snake_seeded_at_one_end(an):
    """a hand-made skeleton at one end of a long thin process: as many sweeps as the far end is hops away.  Catches a loop that ends
    by count and a brick that is not woken across a corner: the far end would stay at 0."""
    import kimimaro_amd
    lab, path = snake()
    assert len(path) > 200
    skel = kimimaro_amd.Skeleton(np.array([path[0], path[3]], dtype=np.float32) * np.asarray(an, dtype=np.float32), segid=300)
    got_f, got_s, stats = assert_same(lab, skel, an)
    assert np.all(got_f[lab != 0] != 0) and got_f[path[-1]] == 2
    assert stats["distance_sweeps"] >= 2 and stats["feature_sweeps"] >= 2
    assert stats["distance_bricks"][0] == stats["bricks"]            # the first sweep visits every brick ...
    assert stats["distance_bricks"][-1] < stats["bricks"]            # ... the last ones only the neighbourhood of what changed


def test_device_tensor_input():
    """a label tensor already on the GPU, indexed [x, y, z]: the same result as the numpy volume"""
    import torch
    import kimimaro_amd
    an = (16, 16, 40)
    lab = two_label_volume()
    want_f, want_s = kimimaro_amd.oversegment(lab, skeletons_for(an), anisotropy=an)
    d = torch.from_numpy(lab.astype(np.int32)).to("cuda")
    got_f, got_s = kimimaro_amd.oversegment(d, skeletons_for(an), anisotropy=an)
    np.testing.assert_array_equal(got_f, want_f)
    for k in want_s:
        np.testing.assert_array_equal(got_s[k].segments, want_s[k].segments)


@pytest.mark.parametrize("an", ANISOTROPIES)
def test_many_source_field_and_feature_map(an):
    """ops.euclidean_distance_field(mask, (n, 3) sources, return_feature_map=True): field bit for bit, feature map exactly"""
    from kimimaro_amd import ops
    mask = random_walk_tube((45, 38, 31), seed=4)
    mask[38:45, 28:38, 0:7] = 0
    mask[40:44, 30:36, 2:5] = 1                              # a part no source lies in, a voxel of background all around it
    pts = np.argwhere(mask[:38])
    sources = np.concatenate([pts[::997], pts[5:6], pts[5:6], np.argwhere(mask == 0)[:1]])     # a double and one on the background
    want_d, want_f = R.geodesic_voronoi((mask != 0).astype(np.int64), [(tuple(int(c) for c in s), j + 1, 1) for j, s in enumerate(sources)], an)
    field, loc, fmap = ops.euclidean_distance_field(mask, sources, anisotropy=an, return_max_location=True, return_feature_map=True)
    assert field.dtype == np.float32 and field.shape == mask.shape
    np.testing.assert_array_equal(field.view(np.uint32), want_d.view(np.uint32))
    np.testing.assert_array_equal(fmap, want_f)
    assert np.all(np.isinf(field[40:44, 30:36, 2:5])) and np.all(fmap[40:44, 30:36, 2:5] == 0)
    finite = np.where(np.isfinite(want_d), want_d, -1)
    assert field[loc] == finite.max() and loc == tuple(np.argwhere(finite.T == finite.max())[0][::-1])
    only = ops.euclidean_distance_field(mask, sources, anisotropy=an)
    np.testing.assert_array_equal(only.view(np.uint32), want_d.view(np.uint32))
