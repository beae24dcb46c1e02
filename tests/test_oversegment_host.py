"""oversegment without a GPU: (a) the CPU reference of the contract (tests/feature_ref.py) checks itself against the contract's
equations, (b) the product exports kimimaro.oversegment's interface, refuses what it does not do before touching a GPU and fails
loudly without one.  (The new C symbols are covered by test_abi.py: header, _abi.SYMBOLS and the library have to agree.)"""
import inspect

import numpy as np
import pytest

import feature_ref as R


class Skel:
    def __init__(self, segid, vertices):
        self.id = segid
        self.vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.extra_attributes = [{"id": "radius", "data_type": "float32", "num_components": 1}]


def two_label_volume():
    """label 7: an L-shaped slab with a detached blob (no vertex there); label 9: a bar; label 3: no skeleton; 5: one voxel"""
    lab = np.zeros((20, 14, 9), dtype=np.uint32, order="F")
    lab[1:15, 1:5, 1:6] = 7
    lab[1:5, 5:12, 1:6] = 7
    lab[16:19, 10:13, 6:8] = 7          # second component of 7
    lab[6:19, 6:9, 2:5] = 9
    lab[8:12, 10:13, 1:3] = 3
    lab[0, 13, 8] = 5
    return lab


def skeletons_for(an):
    an = np.asarray(an, dtype=np.float32)
    return {
        7: Skel(7, np.array([[2, 2, 3], [8, 2, 3], [13, 3, 2], [2, 10, 3], [2, 2, 3], [7, 7, 3]], dtype=np.float32) * an),
        9: Skel(9, np.array([[7, 7, 3], [17, 7, 3], [40, 7, 3]], dtype=np.float32) * an),       # one vertex outside the volume
        5: Skel(5, np.array([[0, 13, 8]], dtype=np.float32) * an),                              # a one-voxel label: skipped
        11: Skel(11, np.array([[3, 3, 3]], dtype=np.float32) * an),                             # its label does not occur
        0: Skel(0, np.array([[9, 11, 2]], dtype=np.float32) * an),                              # id 0: skipped
    }


def fixpoint_residual(ids, dist, anisotropy):
    """max over the voxels of |d(v) - min(0 at d == 0, min over same-label neighbours fl(d(u) + w))| (vectorised numpy: not the heap)"""
    sx, sy, sz = ids.shape
    pad_ids = np.zeros((sx + 2, sy + 2, sz + 2), dtype=np.int64)
    pad_ids[1:-1, 1:-1, 1:-1] = ids
    pad_d = np.full((sx + 2, sy + 2, sz + 2), np.inf, dtype=np.float32)
    pad_d[1:-1, 1:-1, 1:-1] = dist
    best = np.full(ids.shape, np.inf, dtype=np.float32)
    for dx, dy, dz in R.directions():
        w = np.float32(R.step_length((dx, dy, dz), anisotropy))
        sl = (slice(1 + dx, 1 + dx + sx), slice(1 + dy, 1 + dy + sy), slice(1 + dz, 1 + dz + sz))
        cand = np.where((pad_ids[sl] == ids) & (ids != 0), pad_d[sl] + w, np.float32(np.inf)).astype(np.float32)
        best = np.minimum(best, cand)
    return best


@pytest.mark.parametrize("an", [(1, 1, 1), (16, 16, 40), (0.5, 1.25, 3.0)])
def test_reference_satisfies_the_contract(an):
    lab = two_label_volume()
    skels = skeletons_for(an)
    feats, out, (dist, comp, ids) = R.oversegment(lab, skels, an)
    # d: the fixpoint equation at every voxel (a seed is 0, every other voxel the minimum over its same-label neighbours)
    best = fixpoint_residual(ids, dist, an)
    seeds = dist == 0
    assert seeds.sum() == 6                 # 4 distinct voxels of label 7's vertices on label 7 + 2 of label 9's inside the volume
    np.testing.assert_array_equal(dist[~seeds], best[~seeds])
    assert np.all(best[seeds] > 0)
    # background, a label without skeleton, the skipped one-voxel label, the component without a vertex: 0
    assert np.all(feats[lab == 0] == 0) and np.all(feats[lab == 3] == 0) and np.all(feats[lab == 5] == 0)
    assert np.all(feats[16:19, 10:13, 6:8] == 0) and np.all(np.isinf(dist[16:19, 10:13, 6:8]))
    assert np.all(feats[(lab == 9)] != 0) and np.all(feats[1:15, 1:5, 1:6] != 0)
    # provisional numbers: label 7's vertices are 1..6, label 9's 7..9 (skipped skeletons consume none)
    assert set(np.unique(comp[lab == 7])) == {0, 1, 2, 3, 4}               # 5 shares a voxel with 1; 6 sits on label 9: seeds nothing
    assert set(np.unique(comp[lab == 9])) == {7, 8}                        # vertex 9 lies outside the volume
    assert comp[2, 2, 3] == 1                                              # two vertices (1 and 5) on one voxel: the smaller
    # every owned voxel lies in the label of its vertex, and K = number of distinct owners
    K = int(feats.max())
    assert K == len(np.unique(comp[comp != 0])) == 6
    assert feats.dtype == np.uint8
    # renumbered by first appearance in the Fortran raster
    flat = feats.ravel(order="F")
    firsts = [int(np.flatnonzero(flat == k)[0]) for k in range(1, K + 1)]
    assert firsts == sorted(firsts)
    # segments: the final label at every vertex's voxel, 0 outside; inputs untouched, containers kept
    assert isinstance(out, dict) and list(out) == list(skels)
    assert not hasattr(skels[7], "segments") and len(skels[7].extra_attributes) == 1
    assert out[7].segments.dtype == np.uint64 and out[7].segments[0] == out[7].segments[4] == feats[2, 2, 3]
    assert out[7].segments[5] == feats[7, 7, 3] == out[9].segments[0]
    assert out[9].segments[2] == 0 and out[5].segments[0] == 0 and out[11].segments[0] == feats[3, 3, 3]
    assert [a["id"] for a in out[7].extra_attributes] == ["radius", "segments"]


def test_reference_owner_lies_in_the_same_component():
    """every owned voxel's vertex lies in the same label and the same 26-component (scipy's labelling as the judge)"""
    from scipy import ndimage
    lab = two_label_volume()
    an = (1, 1, 1)
    feats, out, (dist, comp, ids) = R.oversegment(lab, skeletons_for(an), an)
    voxel_of = {}
    base = 0
    for key in (7, 9):
        for j, v in enumerate(R.vertex_voxels(skeletons_for(an)[key], an)):
            voxel_of[base + j + 1] = tuple(int(c) for c in v)
        base += 6 if key == 7 else 3
    for L in (7, 9):
        cc, _ = ndimage.label(lab == L, structure=np.ones((3, 3, 3)))
        for number in np.unique(comp[lab == L]):
            if number == 0:
                continue
            v = voxel_of[int(number)]
            assert lab[v] == L
            assert np.all(cc[(comp == number)] == cc[v])


def test_reference_slabs_of_a_box():
    """an isotropic solid box with seeds along its axis: the segments are the slabs between the seeds' mid planes; a voxel on a mid
    plane is equally far from both seeds and goes to the smaller number"""
    lab = np.ones((30, 5, 5), dtype=bool, order="F")
    skel = Skel(1, [[4, 2, 2], [14, 2, 2], [24, 2, 2]])
    feats, out, _ = R.oversegment(lab, skel, (1, 1, 1))
    assert not isinstance(out, (dict, list)) and out.segments.tolist() == [1, 2, 3]
    want = np.zeros((30, 5, 5), dtype=np.uint8)
    want[:10], want[10:20], want[20:] = 1, 2, 3       # x = 9 is 5 from seed 1 and 5 from seed 2 -> 1; x = 19 -> 2
    np.testing.assert_array_equal(feats, want)


def test_reference_list_input_and_numbering_order():
    lab = np.zeros((12, 4, 4), dtype=np.uint64, order="F")
    lab[:6] = 2 ** 40 + 5
    lab[6:] = 3
    a, b = Skel(3, [[9, 1, 1]]), Skel(2 ** 40 + 5, [[4, 1, 1], [1, 1, 1]])
    feats, out, (dist, comp, ids) = R.oversegment(lab, [a, b], (1, 1, 1))
    assert isinstance(out, list) and len(out) == 2
    assert comp[9, 1, 1] == 1 and comp[4, 1, 1] == 2 and comp[1, 1, 1] == 3          # container order decides the provisional numbers
    assert feats[0, 0, 0] == 1 and feats[5, 0, 0] == 2 and feats[11, 0, 0] == 3      # the raster decides the final ones
    assert out[0].segments.tolist() == [3] and out[1].segments.tolist() == [2, 1]


# ---- (b) the product's interface -------------------------------------------------------------------------------------------

def test_oversegment_is_exported_with_the_reference_signature():
    import kimimaro_amd
    sig = inspect.signature(kimimaro_amd.oversegment)
    public = [(n, p.default) for n, p in sig.parameters.items() if not n.startswith("_")]
    assert [n for n, _ in public] == ["all_labels", "skeletons", "anisotropy", "progress", "fill_holes", "in_place", "downsample"]
    assert public[0][1] is inspect.Parameter.empty and public[1][1] is inspect.Parameter.empty
    assert tuple(public[2][1]) == (1, 1, 1)
    assert [d for _, d in public[3:]] == [False, False, False, 0]
    assert all(p.default is not inspect.Parameter.empty for n, p in sig.parameters.items() if n.startswith("_"))


def test_oversegment_refuses_what_it_does_not_do_before_any_gpu_use():
    import kimimaro_amd
    lab = np.ones((4, 4, 4), dtype=np.uint32)
    skel = kimimaro_amd.Skeleton([[1, 1, 1]], segid=1)
    with pytest.raises(NotImplementedError, match="downsample"):
        kimimaro_amd.oversegment(lab, skel, downsample=1)
    with pytest.raises(NotImplementedError, match="fill_holes"):
        kimimaro_amd.oversegment(lab, skel, fill_holes=True)


def test_oversegment_fails_loudly_without_gpu():
    import torch
    import kimimaro_amd
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lab = np.ones((4, 4, 4), dtype=np.uint32)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.oversegment(lab, kimimaro_amd.Skeleton([[1, 1, 1]], segid=1))
    from kimimaro_amd import ops
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        ops.euclidean_distance_field(lab, [[1, 1, 1], [2, 2, 2]], return_feature_map=True)


def test_many_source_field_takes_the_reference_keyword():
    from kimimaro_amd import ops
    p = inspect.signature(ops.euclidean_distance_field).parameters
    assert p["return_feature_map"].default is False and list(p)[:2] == ["labels", "source"]
