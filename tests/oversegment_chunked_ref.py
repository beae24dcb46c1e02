"""What the host tests of oversegment_chunked put in place of the GPU, and the small datasets both tiers share.

* relax_box: the `_box` seam as numpy Jacobi sweeps over the 26 directions -- every voxel of a box takes, from the values of the
  sweep before, the minimum over its same-label neighbours INSIDE THE BOX of fl(d(u) + w) in float32 (phase 1), or the smallest
  number among the neighbours with fl(d(u) + w) == d(v) (phase 2), until a sweep changes nothing.  The weights are
  feature_ref.step_length's.  It knows nothing of cores, halos or rounds: those are the driver's.
* the datasets: random blobs with holes, the serpentine, the U, the tie and skip-rule volumes, each with its skeletons.
* CASES: (name, builder) pairs that the host file runs through the seam and the GPU file through the kernels.
"""
import numpy as np

import feature_ref as R

NONE = 0xFFFFFFFF
ANISOTROPIES = [(1, 1, 1), (16, 16, 40), (4, 4, 40), (1.5, 1, 3)]


class Skel:
    def __init__(self, segid, vertices):
        self.id = segid
        self.vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.extra_attributes = [{"id": "radius", "data_type": "float32", "num_components": 1}]


def skel(segid, voxels, an=(1, 1, 1)):
    """a skeleton whose vertices are these voxels (physical space)"""
    return Skel(segid, np.asarray(voxels, dtype=np.float32).reshape(-1, 3) * np.asarray(an, dtype=np.float32))


def _shifted(pad, step, shape):
    return pad[tuple(slice(1 + d, 1 + d + n) for d, n in zip(step, shape))]


def relax_box(labels, d, f, anisotropy, phase):
    """the `_box` seam of post.oversegment_chunked on host arrays [x, y, z]"""
    labels = np.asarray(labels)
    shape = labels.shape
    pad_l = np.zeros(tuple(n + 2 for n in shape), dtype=labels.dtype)
    pad_l[1:-1, 1:-1, 1:-1] = labels
    steps = [(s, np.float32(R.step_length(s, anisotropy)), (_shifted(pad_l, s, shape) == labels) & (labels != 0)) for s in R.directions()]
    d = np.array(d, dtype=np.float32)
    pad_d = np.full(pad_l.shape, np.inf, dtype=np.float32)
    if phase == 1:
        while True:
            pad_d[1:-1, 1:-1, 1:-1] = d
            new = d.copy()
            for s, w, same in steps:
                cand = (_shifted(pad_d, s, shape) + w).astype(np.float32)
                new = np.where(same & (cand < new), cand, new)
            if np.array_equal(new, d):
                return d
            d = new
    pad_d[1:-1, 1:-1, 1:-1] = d
    open_ = (d > 0) & np.isfinite(d)                                       # a seed keeps its number; nothing reaches an infinite voxel
    achieving = [(s, same & open_ & ((_shifted(pad_d, s, shape) + w).astype(np.float32) == d)) for s, w, same in steps]
    f = np.array(f, dtype=np.uint32)
    pad_f = np.full(pad_l.shape, NONE, dtype=np.uint32)
    while True:
        pad_f[1:-1, 1:-1, 1:-1] = f
        new = f.copy()
        for s, edge in achieving:
            cand = _shifted(pad_f, s, shape)
            new = np.where(edge & (cand < new), cand, new)
        if np.array_equal(new, f):
            return f
        f = new


# ---- datasets ----------------------------------------------------------------------------------------------------------------
def random_blobs(rng, shape, nlabels=4, nseeds=9, an=(1, 1, 1), dtype=np.uint32):
    """`nlabels` labels painted as overlapping boxes, with holes punched into them; `nseeds` vertices on random label voxels,
    one skeleton per label in descending label order (the container order is not the label order)"""
    lab = np.zeros(shape, dtype=dtype, order="F")
    ext = np.array(shape)
    for L in range(1, nlabels + 1):
        for _ in range(3):
            lo = rng.integers(0, np.maximum(ext - 2, 1))
            hi = np.minimum(lo + rng.integers(2, np.maximum(ext // 2 + 2, 3)), ext)
            lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = L
    lab[rng.random(shape) < 0.15] = 0
    pts = np.argwhere(lab != 0)
    pick = pts[rng.choice(len(pts), size=min(nseeds, len(pts)), replace=False)]
    skels = {}
    for L in range(nlabels, 0, -1):
        mine = [p for p in pick if lab[tuple(p)] == L]
        if mine:
            skels[L] = skel(L, mine, an)
    return lab, skels


def serpentine(rows, sx):
    """rows of label 7 at y = 0, 2, 4, ..., joined alternately at x = sx - 1 and x = 0: a cut at sx / 2 is crossed once per row"""
    lab = np.zeros((sx, 2 * rows - 1, 1), dtype=np.uint16, order="F")
    for r in range(rows):
        lab[:, 2 * r, 0] = 7
        if r + 1 < rows:
            lab[sx - 1 if r % 2 == 0 else 0, 2 * r + 1, 0] = 7
    return lab


def u_turn():
    """a U of label 4 whose two arms lie in core A (x < 6) and whose bend lies in core B: from a seed at the end of one arm the other
    arm is reached only through B -- with chunks (6, 9, 3), two cores"""
    lab = np.zeros((12, 7, 3), dtype=np.uint8, order="F")
    lab[1:11, 1, 1] = 4
    lab[1:11, 5, 1] = 4
    lab[10, 1:6, 1] = 4
    return lab, skel(4, [[1, 1, 1]])


def tie_volume():
    """label 2: a bar along x whose two seeds meet exactly on the cut plane x = 8 (chunks of 8); label 3: a plate in which two seeds
    on a diagonal meet on the grid edge x = y = 8; label 5: a block in which two seeds on a space diagonal meet at the grid corner
    (8, 8, 8).  Per label the later-listed vertex sits on the low side: the smaller number has to win all the same."""
    lab = np.zeros((16, 16, 16), dtype=np.uint32, order="F")
    lab[3:14, 1, 1] = 2                       # seeds at x = 3 and x = 13: equally far from x = 8
    lab[4:13, 4:13, 3] = 3                    # seeds at (5, 5) and (11, 11): the voxel (8, 8) is three diagonal steps from both
    lab[5:12, 5:12, 5:12] = 5                 # seeds at (6, 6, 6) and (10, 10, 10): (8, 8, 8) two diagonal steps from both
    return lab, [skel(2, [[13, 1, 1], [3, 1, 1]]), skel(3, [[11, 11, 3], [5, 5, 3]]), skel(5, [[10, 10, 10], [6, 6, 6]])]


def numbering_volume():
    """two labels whose first voxels in the DATASET raster (x fastest) come in the opposite order of the cores that hold them: with
    chunks (4, 8, 1) core 0 is x < 4 and core 1 x >= 4; label 9 starts at (5, 0) -- raster index 5, core 1 --, label 8 at (0, 1) --
    raster index 8, core 0"""
    lab = np.zeros((8, 3, 1), dtype=np.uint32, order="F")
    lab[5:8, 0, 0] = 9
    lab[0:3, 1, 0] = 8
    return lab, [skel(8, [[1, 1, 0]]), skel(9, [[6, 0, 0]])]


def long_line():
    """a 300-voxel line with a vertex on every voxel: K = 300 needs uint16"""
    lab = np.zeros((300, 2, 2), dtype=np.uint8, order="F")
    lab[:, 0, 0] = 1
    return lab, skel(1, [[x, 0, 0] for x in range(300)])


def skip_volume(an=(1, 1, 1)):
    """every skip rule with the cut x = 6 of chunks (6, 5, 4) nearby"""
    lab = np.zeros((12, 5, 4), dtype=np.uint32, order="F")
    lab[2:10, 1, 1] = 7                       # crosses the cut
    lab[5, 3, 1] = 5                          # one voxel in the whole dataset: skipped
    lab[5, 3, 3] = 6                          # one voxel in EACH of two cores, touching across the cut: not skipped
    lab[6, 3, 3] = 6
    lab[4:8, 4, 0] = 3                        # a label without a skeleton
    skels = {
        7: skel(7, [[3, 1, 1], [8, 1, 1], [3, 1, 1], [6, 3, 3], [40, 1, 1], [6, 1, 1]], an),     # double, off its label, outside, on the cut
        5: skel(5, [[5, 3, 1]], an),
        6: skel(6, [[5, 3, 3]], an),
        11: skel(11, [[5, 1, 1]], an),        # its label does not occur
        0: skel(0, [[5, 4, 0]], an),          # id 0
    }
    return lab, skels


def wide_labels():
    """uint64 labels above 2^32 that differ only in their high words, side by side across the cut x = 5"""
    lab = np.zeros((10, 4, 3), dtype=np.uint64, order="F")
    lab[1:9, 1, 1] = (1 << 40) + 5
    lab[1:9, 2, 1] = (2 << 40) + 5
    return lab, [skel((2 << 40) + 5, [[2, 2, 1], [7, 2, 1]]), skel((1 << 40) + 5, [[7, 1, 1]])]


def bool_volume():
    lab = np.zeros((11, 6, 5), dtype=bool, order="F")
    lab[1:10, 1:5, 1:4] = True
    lab[4:6, 2:4, 1:4] = False
    return lab, {3: skel(0, [[2, 2, 2]]), 4: skel(12345, [[8, 3, 2], [5, 1, 1]])}


def plane_volume():
    """two axes"""
    lab = np.zeros((13, 9), dtype=np.uint16, order="F")
    lab[1:12, 1:8] = 300
    lab[5:8, 3:6] = 0
    return lab, skel(300, [[1, 1, 0], [11, 7, 0], [6, 1, 0]])


# (name, builder -> (dataset, skeletons, anisotropy, chunk_shape)): run through the seam by the host file, through the kernels by
# the GPU file
CASES = [
    ("serpentine", lambda: (serpentine(6, 16), skel(7, [[0, 0, 0]]), (1, 1, 1), (8, 64, 1))),
    ("u_turn", lambda: u_turn() + ((1, 1, 1), (6, 9, 3))),
    ("ties", lambda: tie_volume() + ((1, 1, 1), (8, 8, 8))),
    ("numbering", lambda: numbering_volume() + ((1, 1, 1), (4, 8, 1))),
    ("skips", lambda: skip_volume() + ((1, 1, 1), (6, 5, 4))),
    ("skips_anisotropic", lambda: skip_volume((16, 16, 40)) + ((16, 16, 40), (6, 3, 2))),
    ("uint64", lambda: wide_labels() + ((4, 4, 40), (5, 4, 3))),
    ("bool", lambda: bool_volume() + ((1.5, 1, 3), (4, 4, 4))),
    ("two_axes", lambda: plane_volume() + ((1, 1, 1), (5, 4))),
    ("one_box", lambda: skip_volume() + ((1, 1, 1), (64, 64, 64))),
]


def assert_skeletons(got, want, original):
    assert type(got) is type(want)
    if isinstance(want, dict):
        assert list(got) == list(want)
    for g, w, o in zip(R.skeleton_list(got), R.skeleton_list(want), R.skeleton_list(original)):
        assert g is not o and not hasattr(o, "segments")
        assert g.segments.dtype == np.uint64 and g.segments.shape == (len(g.vertices),)
        np.testing.assert_array_equal(g.segments, w.segments)
        np.testing.assert_array_equal(g.vertices, o.vertices)
        assert [a for a in g.extra_attributes if a["id"] == "segments"] == [{"id": "segments", "data_type": "uint64", "num_components": 1}]
        assert not any(a["id"] == "segments" for a in o.extra_attributes)            # the input skeletons are untouched
