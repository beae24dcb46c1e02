"""The statement of DESIGN.md 3.21 for a dataset in boxes, written out with loops on tests/chunked_ref.py and tests/graph_ref.py: the
boxes of a dataset, per box the CLIPPED slice of the dataset's voxel graph (or the graph of the supervoxel box alone), the placement
of a fragment, and the composition that skeletonize_graph_chunked is defined as.  numpy only: what skeletonizes a box and what
postprocesses a fused skeleton are handed in."""
import functools

import numpy as np

import chunked_ref as R
import graph_ref as G


def fragments(lab, chunk_shape, run, graph=None, supervoxels=None, merges=None, dust_threshold=R.CHUNK_DUST, **kwargs):
    """{label: [placed fragments in chunk order]}, labels ascending; run(box labels, voxel_graph=, **kwargs of skeletonize)"""
    assert (graph is None) != (supervoxels is None)
    out = {}
    for _, _, lo, hi in R.boxes(lab.shape, chunk_shape):
        cut = tuple(slice(a, b) for a, b in zip(lo, hi))
        box_graph = G.clip(graph[cut]) if graph is not None else G.graph_of(supervoxels[cut], 26, merges)
        res = run(lab[cut], teasar_params=R.TP, anisotropy=R.AN, fix_borders=True, fix_branching=True, dust_threshold=dust_threshold,
                  voxel_graph=box_graph, **kwargs)
        for label, skel in res.items():
            if not skel.empty():
                out.setdefault(label, []).append(R.placed(skel, lo, label))
    return {label: out[label] for label in sorted(out)}


compose = R.compose


@functools.lru_cache(maxsize=None)
def walled_graph():
    """(graph, label, axis, at): the graph of R.dataset(0) with a wall across its largest label, through the label's middle along x but
    at least three voxels away from every cut of the dataset's chunk grid"""
    lab = R.dataset(0)
    values, counts = np.unique(lab[lab != 0], return_counts=True)
    label = int(values[int(np.argmax(counts))])
    xs = np.flatnonzero((lab == label).any(axis=(1, 2)))
    cuts = sorted({b[3][0] - 1 for b in R.boxes(lab.shape, R.DATASETS[0][3])} | {b[2][0] for b in R.boxes(lab.shape, R.DATASETS[0][3])})
    inner = [int(x) for x in xs[2:-3] if all(abs(int(x) - c) >= 3 for c in cuts)]
    at = min(inner, key=lambda x: abs(x - int(xs[len(xs) // 2])))
    g = G.graph_of(lab, 26, None)
    only = G.wall(g, 0, at)
    mine = lab == label
    g[mine] = only[mine]                       # (the wall stands inside the one label only)
    g.setflags(write=False)
    return g, label, 0, at


@functools.lru_cache(maxsize=None)
def u_shape():
    """(labels, supervoxels, merges): one label (7) shaped as a U in a (48, 40, 24) volume whose two arms touch along a stretch --
    arm A = supervoxel 1, arm B = supervoxel 2, the bend = supervoxel 3; merges joins each arm to the bend, not the arms."""
    sv = np.zeros((48, 40, 24), dtype=np.uint32, order="F")
    sv[4:40, 8:20, 6:18] = 1                   # arm A along x
    sv[4:40, 20:32, 6:18] = 2                  # arm B along x, touching arm A on the plane between y = 19 and y = 20
    sv[10:40, 17:23, 6:18] = 0                 # ... apart again except for x in [4, 10): the stretch where they touch
    sv[40:46, 8:32, 6:18] = 3                  # the bend joins the two arms at their far end
    lab = np.where(sv != 0, 7, 0).astype(np.uint32, order="F")
    lab.setflags(write=False)
    sv.setflags(write=False)
    return lab, sv, ((1, 3), (2, 3))
