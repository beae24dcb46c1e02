"""What the tests of fill_all_holes_chunked share, on the statements of tests/fill_ref.py and the datasets of
tests/section_filled_chunked_ref.py: numpy and scipy only, independent of the product.

  apply_on_host     the _apply hook: fill_ref.owner_volume on a core, its ids taken relative to the core's base
  fill_on_host      fill_all_holes_chunked with both hooks: nothing touches the GPU
  by_cores          every core filled on its own (fill_ref.static) and put together again: what the per-box route computes
  assert_same_fill  volume, count and the state of every label against fill_ref.static of the whole
Also the datasets beyond those of section_filled_chunked_ref."""
import numpy as np

import fill_ref
import section_filled_chunked_ref as H

BIG = 2 ** 63 + 5                     # a label with the top bit set: the last in the order of unsigned words
CORES_2D = (10, 8)


def apply_on_host(core, ids, base, owner):
    r = ids.astype(np.int64) - int(base)
    assert core.dtype.kind == "u" and ids.dtype == np.uint32 and owner.dtype == np.uint64 and owner[0] == 0
    assert r.min() >= 1 and r.max() < owner.size
    return fill_ref.owner_volume(core, owner, r), int(np.count_nonzero(owner[r]))


def fill_on_host(dataset, chunk_shape=H.CORES, **kwargs):
    from kimimaro_amd import post
    return post.fill_all_holes_chunked(dataset, chunk_shape, _regions=H.regions_on_host, _apply=apply_on_host, **kwargs)


def core_slices(shape, chunk_shape):
    from kimimaro_amd.plan import halo_boxes
    lo, hi, _, _ = halo_boxes(shape, chunk_shape, 0)
    return [tuple(slice(int(a), int(b)) for a, b in zip(l, h))[:len(shape)] for l, h in zip(lo, hi)]


def by_cores(dataset, chunk_shape=H.CORES):
    out = np.array(dataset, copy=True)
    for cut in core_slices(dataset.shape, chunk_shape):
        out[cut] = fill_ref.static(dataset[cut])[0]
    return out


def states(stats):
    return dict(zip(stats["label_value"].tolist(), stats["label_state"].tolist()))


def assert_same_fill(got, count, stats, dataset):
    """-> fill_ref.static(dataset), after holding the driver's result against it"""
    want = fill_ref.static(dataset)
    assert got.dtype == dataset.dtype and got.shape == dataset.shape
    np.testing.assert_array_equal(got, want[0])
    assert count == want[1] == stats["filled"]
    assert states(stats) == want[2] and stats["labels"] == len(want[2])
    return want


def swapped_nested_shells():
    """nested_shells with the labels 3 and 4 exchanged: the inner shell has its turn first and the outer one paints over its fill"""
    lab = H.nested_shells()
    return np.asfortranarray(np.where(lab == 3, 4, np.where(lab == 4, 3, lab)).astype(lab.dtype))


def bool_dataset():
    return np.asfortranarray(H.straddling_shells()["corner"] != 0)


def uint64_dataset():
    """nested_shells with the outer shell as BIG, the inner one 7 and the core 2^40: 7 fills first, BIG last and over it"""
    lab = H.nested_shells()
    out = np.zeros(lab.shape, dtype=np.uint64, order="F")
    out[lab == 3], out[lab == 4], out[lab == 6] = BIG, 7, 2 ** 40
    return out


def ring_2d():
    """two axes: a ring of label 9 across the cuts x = 10 and y = 8 with a dot of label 2 in it, closed as a 2-D image"""
    lab = np.zeros(H.SHAPE[:2], dtype=np.uint8, order="F")
    lab[6:15, 4:12] = 9
    lab[7:14, 5:11] = 0
    lab[9:11, 7:9] = 2
    return lab


def flat_dataset():
    """the ring with a unit z axis: three axes, so every voxel lies on a face and nothing is a hole"""
    return np.asfortranarray(ring_2d()[:, :, None])
