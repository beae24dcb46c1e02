"""The statement of DESIGN.md 3.15 written out with loops (the boxes of a dataset, the placement of a fragment, the composition that
skeletonize_chunked is defined as) and the two datasets of the chunked tests.  numpy only: what skeletonizes a box and what
postprocesses a fused skeleton are handed in."""
import functools

import numpy as np

from kimimaro_amd.skeleton import Skeleton

AN = (16, 16, 40)
TP = {"scale": 1.5, "const": 300, "pdrf_scale": 100000, "pdrf_exponent": 4, "soma_acceptance_threshold": 3500,
      "soma_detection_threshold": 1100, "soma_invalidation_const": 300, "soma_invalidation_scale": 2}
# shape, labels, seed, chunk_shape, chunks, labels that lie in more than one chunk at least
DATASETS = (((96, 80, 48), 14, 11, (48, 40, 48), 4, 12),
            ((100, 70, 40), 10, 5, (48, 48, 48), 6, 10))
CHUNK_DUST, POST_DUST, TICK = 300, 1000, 1500
GLOBAL_DUST = 12000              # dataset 0: 8 labels pass it chunk by chunk, 12 in the whole dataset; 1003 and 1012 never do


@functools.lru_cache(maxsize=None)
def dataset(k):
    from shapes import voronoi_labels
    shape, nlabels, seed = DATASETS[k][:3]
    lab = voronoi_labels(shape, nlabels, seed, pts_per_label=6, step=10.0, anisotropy=AN)
    lab.setflags(write=False)
    return lab


def axis_boxes(n, c):
    """[(start, core end, box end)] of one axis"""
    starts = [0]
    while starts[-1] + c < n - 1:
        starts.append(starts[-1] + c)
    return [(a, starts[i + 1] if i + 1 < len(starts) else n, min(a + c + 1, n)) for i, a in enumerate(starts)]


def boxes(shape, chunk_shape):
    """[(core low, core high, box low, box high)], x fastest, then y, then z"""
    cuts = [axis_boxes(n, c) for n, c in zip(shape, chunk_shape)]
    return [((x[0], y[0], z[0]), (x[1], y[1], z[1]), (x[0], y[0], z[0]), (x[2], y[2], z[2]))
            for z in cuts[2] for y in cuts[1] for x in cuts[0]]


def placed(skel, low, label, anisotropy=AN):
    an = np.asarray(anisotropy, dtype=np.float32)
    voxel = np.rint(skel.vertices.astype(np.float64) / an.astype(np.float64)).astype(np.int64)
    assert np.array_equal(voxel.astype(np.float32) * an, skel.vertices)
    v = (voxel + np.asarray(low, dtype=np.int64)).astype(np.float32) * an
    return Skeleton(v, skel.edges.copy(), skel.radii.copy(), skel.vertex_types.copy(), segid=label, transform=skel.transform.copy(),
                    space="physical")


def fragments(lab, chunk_shape, run, dust_threshold=CHUNK_DUST, dust_global=False, targets_after=(), **kwargs):
    """{label: [placed fragments in chunk order]}, labels ascending; run(box labels, **kwargs of skeletonize) -> {label: Skeleton}"""
    kept = None
    if dust_global:
        values, counts = np.unique(lab, return_counts=True)
        kept = {int(v) for v, c in zip(values, counts) if v != 0 and c > dust_threshold}
    out = {}
    for _, _, lo, hi in boxes(lab.shape, chunk_shape):
        box = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        kw = dict(kwargs, dust_threshold=dust_threshold)
        if kept is not None:
            ids = sorted(kept & set(np.unique(box).tolist()))
            if not ids:
                continue
            kw.update(dust_threshold=0, object_ids=ids)
        inside = [tuple(int(p[a] - lo[a]) for a in range(3)) for p in targets_after if all(lo[a] <= p[a] < hi[a] for a in range(3))]
        res = run(box, teasar_params=TP, anisotropy=AN, fix_borders=True, fix_branching=True, extra_targets_after=inside, **kw)
        for label, skel in res.items():
            if not skel.empty():
                out.setdefault(label, []).append(placed(skel, lo, label))
    return {label: out[label] for label in sorted(out)}


def fused(frags):
    return {label: Skeleton.simple_merge(f).consolidate() for label, f in frags.items()}


def compose(frags, postprocess, dust_threshold=POST_DUST, tick_threshold=TICK):
    """{label: postprocess(fused fragments)}, the empty results dropped"""
    out = {label: postprocess(skel, dust_threshold, tick_threshold) for label, skel in fused(frags).items()}
    return {label: skel for label, skel in out.items() if not skel.empty()}


def assert_same(got, want, radii_rtol=None):
    assert list(got) == list(want)
    for label in want:
        a, b = got[label], want[label]
        assert a.id == label and a.space == "physical"
        np.testing.assert_array_equal(a.vertices, b.vertices)
        np.testing.assert_array_equal(a.edges, b.edges)
        if radii_rtol is None:
            np.testing.assert_array_equal(a.radii, b.radii)
        else:
            np.testing.assert_allclose(a.radii, b.radii, rtol=radii_rtol)
