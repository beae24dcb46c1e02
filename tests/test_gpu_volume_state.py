"""The state that goes with a component volume on the MI355X: the u16 copy kh_ccl26 makes travels with the tensor Engine.ccl_device
returns (Engine.narrow / Engine.edited), Engine.label_stats returns everything it computed (kimimaro_amd.plan.LabelStats), and
Engine.box is the one way to look at a box of a device volume.  The engine itself keeps nothing of a volume."""
import gc
import os
import sys
import weakref
from collections import defaultdict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def _same_ids(eng, d16, d_cc):
    t = eng.torch
    return d16.element_size() == 2 and d16.numel() == d_cc.numel() and bool(t.equal(d16.to(t.int32) & 0xFFFF, d_cc))


def _skeletons(eng, cc, n, remap, dust, **kw):
    import kimimaro_amd
    from kimimaro_amd import intake
    empty = defaultdict(list)
    return intake.skeletonize_cc(eng, cc, n, remap, dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS), np.ones(3, dtype=np.float32), dust, True,
                                 True, empty, empty, black_border=False, **kw)


def _find_objects(lab):
    import scipy.ndimage
    return [None if b is None else (tuple(s.start for s in b), tuple(s.stop for s in b)) for b in scipy.ndimage.find_objects(lab)]


def test_the_copy_travels_with_the_tensor(eng):
    lab = np.zeros((16, 12, 8), dtype=np.uint32, order="F")
    lab[0:5, 0:5, 0:5], lab[7:12, 2:9, 1:6], lab[13:16, 9:12, 6:8] = 4, 9, 4
    d_cc, n, _ = eng.ccl(lab)
    assert n == 3
    d16, nbytes = eng.narrow(d_cc)
    assert nbytes == 2 and _same_ids(eng, d16, d_cc)
    other = np.zeros((8, 8, 8), dtype=np.uint32, order="F")
    other[1:7, 1:7, 1:7] = 5
    d_other, n_other, _ = eng.ccl(other)
    assert n_other == 1 and eng.narrow(d_other)[1] == 2
    again, nbytes = eng.narrow(d_cc)
    assert again is d16 and nbytes == 2 and _same_ids(eng, d16, d_cc)
    clone = d_cc.clone()
    got, nbytes = eng.narrow(clone)
    assert got is clone and nbytes == 4
    assert eng.narrow(None) == (None, 4)
    stats = eng.label_stats(d16, 2, eng.torch.zeros(lab.size, dtype=eng.torch.float32, device=eng.device), lab.shape, n)
    assert sorted(stats.counts.tolist()) == [0, 18, 125, 175]
    # after two ccl calls and a label_stats: the engine has no record of a volume's u16 copy or of its boxes
    assert [name for name in vars(eng) if "narrow" in name or "yz" in name] == []


def _shell_and_pit():
    """a hollow 7 x 7 x 7 shell of label 1, a 3 x 3 x 3 block of label 2 inside, one empty voxel layer between them"""
    lab = np.zeros((12, 12, 12), dtype=np.uint32, order="F")
    lab[2:9, 2:9, 2:9] = 1
    lab[3:8, 3:8, 3:8] = 0
    lab[4:7, 4:7, 4:7] = 2
    return lab


@pytest.mark.parametrize("route", ["loop", "one_pass"])
def test_in_place_edits_drop_the_copy(eng, route):
    from kimimaro_amd import intake
    lab = _shell_and_pit()
    shape = lab.shape
    d_cc, n, remap = intake.compute_cc_labels_device(eng, lab)
    assert n == 2 and remap == {1: 1, 2: 2} and eng.narrow(d_cc)[1] == 2
    filled = intake.fill_all_holes_device(eng, d_cc, shape, n) if route == "loop" else eng.fill_all_holes(d_cc, 4, shape)
    assert filled > 0
    got, nbytes = eng.narrow(d_cc)
    assert got is d_cc and nbytes == 4
    assert np.array_equal(eng.to_host_volume(d_cc, shape) != 0, np.pad(np.ones((7, 7, 7), dtype=bool), ((2, 3),) * 3))
    out = _skeletons(eng, intake.LazyVolume(eng, d_cc, shape), n, remap, 0, d_cc=d_cc)
    assert list(out) == [1]             # (a stale u16 copy still holds label 2's 27 voxels)


def test_the_65536_boundary(eng):
    lab = np.zeros((128, 64, 64), dtype=np.uint32, order="F")
    lab[::2, ::2, ::2] = np.arange(1, 65537, dtype=np.uint32).reshape(64, 32, 32)
    d_cc, n, _ = eng.ccl(lab)
    assert n == 65536
    got, nbytes = eng.narrow(d_cc)
    assert got is d_cc and nbytes == 4
    lab[64, 32, 32] = 0
    d_cc, n, _ = eng.ccl(lab)
    assert n == 65535
    d16, nbytes = eng.narrow(d_cc)
    assert nbytes == 2 and _same_ids(eng, d16, d_cc)


@pytest.mark.parametrize("pass_d_cc", [False, True])
def test_nothing_outlives_skeletonize_cc(eng, pass_d_cc):
    from kimimaro_amd import intake
    lab = np.zeros((32, 32, 16), dtype=np.uint32, order="F")
    lab[1:15, 1:31, 1:15], lab[17:31, 1:31, 1:15] = 3, 8
    d_cc, n, remap = intake.compute_cc_labels_device(eng, lab)
    assert n == 2
    d16, nbytes = eng.narrow(d_cc)
    assert nbytes == 2
    refs = [weakref.ref(d_cc), weakref.ref(d16)]
    del d16
    cc = intake.LazyVolume(eng, d_cc, lab.shape)
    if pass_d_cc:
        out = _skeletons(eng, cc, n, remap, 100, d_cc=d_cc)
        del d_cc
    else:
        del d_cc
        out = _skeletons(eng, cc, n, remap, 100)
    assert sorted(out) == [3, 8]
    del cc
    gc.collect()
    assert [r() for r in refs] == [None, None]


def test_nothing_outlives_connect_points(eng):
    from kimimaro_amd import intake
    t = eng.torch
    bar = np.zeros((16, 8, 8), dtype=bool, order="F")
    bar[1:15, 3:5, 3:5] = True

    def allocated():
        skel = intake.connect_points(bar, (1, 3, 3), (14, 4, 4))
        assert len(skel.vertices) >= 2
        del skel
        gc.collect()
        return t.cuda.memory_allocated(eng.device)

    first = allocated()                 # (warms the caches of the shared engine)
    assert allocated() == first


def test_label_stats_on_the_device(eng):
    from kimimaro_amd.plan import LabelStats
    shape = (70, 9, 5)                  # sx > 64: a row crosses a wave
    lab = np.zeros(shape, dtype=np.uint32, order="F")
    lab[3:69, 1:4, 0:2], lab[60:70, 5:9, 2:5] = 1, 2
    lab[65, 2, 1] = 0
    dbf = np.asfortranarray(np.random.default_rng(5).random(shape).astype(np.float32))
    got = eng.label_stats(eng.to_device(lab), 4, eng.to_device(dbf), shape, 2)
    want = prep_ref.label_stats(lab, dbf, 2)
    assert isinstance(got, LabelStats)
    for name, g, w in zip(got._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name
    assert [got.bbox(label) for label in (1, 2)] == _find_objects(lab)


def test_box_and_crop(eng):
    shape = (13, 11, 7)
    vol = np.asfortranarray(np.random.default_rng(7).integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32))
    d = eng.to_device(vol)
    for lo, hi in (((2, 0, 3), (13, 6, 7)), ((12, 10, 6), (13, 11, 7))):
        want = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        view = eng.box(d, shape, lo, hi)
        assert view.device == d.device and tuple(view.shape) == want.shape[::-1]
        assert np.array_equal(view.contiguous().cpu().numpy().view(np.uint32).transpose(2, 1, 0), want)
        assert np.array_equal(eng.crop(d, shape, lo, hi), want)
    assert eng.box(d, shape, (0, 0, 0), shape).data_ptr() == d.data_ptr()      # (a view of the volume, not a copy)
