"""The numpy statement of kh_part_clusters (include/kimi_hip.h): which parts of a group are connected through pairs
of bounding boxes nearer than the group's bound.  All pairs, float64 in the stated operation order, union by minimum.  No GPU, no
library."""
import numpy as np


def boxes_of(vertices):
    """vertex arrays [k, 3] -> f32 [n, 6]: (min x, y, z, max x, y, z) of every part"""
    out = np.zeros((len(vertices), 6), dtype=np.float32)
    for k, v in enumerate(vertices):
        v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
        out[k, :3] = v.min(axis=0)
        out[k, 3:] = v.max(axis=0)
    return out


def axis_gap(lo_a, hi_a, lo_b, hi_b):
    """the distance of two intervals: max(lo_a - hi_b, lo_b - hi_a) where that is positive, else 0"""
    g1 = lo_a - hi_b
    g2 = lo_b - hi_a
    g = np.where(g1 > g2, g1, g2)
    return np.where(g > 0.0, g, 0.0)


def low(a, b):
    """a: f32 [m, 6], b: f32 [n, 6] -> f64 [m, n]: (gx*gx + gy*gy) + gz*gz of every pair, each operation rounded in float64"""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    g = [axis_gap(a[:, None, k], a[:, None, 3 + k], b[None, :, k], b[None, :, 3 + k]) for k in range(3)]
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def near_pairs(boxes, bound2, rows=256):
    """the pairs (t, q), t < q, of one group with low(t, q) < bound2, as an int64 array [m, 2]"""
    n = boxes.shape[0]
    found = []
    for r0 in range(0, n, rows):
        t, q = np.nonzero(low(boxes[r0:r0 + rows], boxes) < bound2)
        t += r0
        keep = t < q
        found.append(np.stack([t[keep], q[keep]], axis=1))
    return np.concatenate(found) if found else np.zeros((0, 2), dtype=np.int64)


def clusters(boxes, group_start, bound2):
    """boxes f32 [n, 6], group_start [G + 1], bound2 f64 [G] -> cluster u32 [n]: the smallest part index, in the numbering of
    `boxes`, among the parts connected to the part through near pairs of its group"""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 6)
    group_start = np.asarray(group_start, dtype=np.int64)
    out = np.arange(boxes.shape[0], dtype=np.int64)
    for g in range(group_start.size - 1):
        p0, p1 = int(group_start[g]), int(group_start[g + 1])
        parent = list(range(p1 - p0))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for t, q in near_pairs(boxes[p0:p1], float(bound2[g])).tolist():
            a, b = find(t), find(q)
            if a != b:
                parent[max(a, b)] = min(a, b)             # the root of a tree is its smallest member
        out[p0:p1] = [p0 + find(x) for x in range(p1 - p0)]
    return out.astype(np.uint32)


def sizes_of(cluster):
    """cluster ids -> the sizes of the clusters, descending"""
    return np.sort(np.unique(np.asarray(cluster), return_counts=True)[1])[::-1]
