"""The numpy statement of DESIGN.md 3.14 (the tables of kh_part_gaps, the merge plan of kh_host_join_plan, the skeleton that
join_close_components_many returns) and the fragment generator of the join tests.  Brute force, no GPU, no library."""
import numpy as np

from kimimaro_amd.skeleton import Skeleton

NONE = 0xFFFFFFFF


def parts_of(skeletons):
    """kimimaro_amd/post.py:56-61: the components of every skeleton in order, consolidated, the empty ones dropped"""
    if isinstance(skeletons, Skeleton):
        skeletons = [skeletons]
    parts = []
    for s in skeletons:
        parts.extend(c.consolidate(remove_disconnected_vertices=True) for c in s.components())
    return [p for p in parts if not p.empty()]


def pair_record(tree, query, bound2=np.inf):
    """(d2, kt, kq, tree_tie) of tree vertices f32 [nt, 3] and query vertices f32 [nq, 3]; (inf, NONE, NONE, False) for none.
    tree_tie: more than one tree vertex attains the minimum for the winning query vertex."""
    t = np.asarray(tree, dtype=np.float32).astype(np.float64)
    q = np.asarray(query, dtype=np.float32).astype(np.float64)
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz                     # [kq, kt]; every operation rounded in f64
    flat = int(np.argmin(d2))                              # the first minimum in (kq, kt) raster order
    kq, kt = divmod(flat, d2.shape[1])
    best = d2[kq, kt]
    if not best < bound2:
        return np.inf, NONE, NONE, False
    return float(best), kt, kq, int(np.count_nonzero(d2[kq] == best)) > 1


def records(vertices, bound2=np.inf):
    """vertices: the parts' vertex arrays -> (d2 f64 [n, n], idx u32 [n, n, 2] = (kt, kq), tree_tie bool [n, n]); row = tree part"""
    n = len(vertices)
    d2 = np.full((n, n), np.inf, dtype=np.float64)
    idx = np.full((n, n, 2), NONE, dtype=np.uint32)
    tie = np.zeros((n, n), dtype=bool)
    for t in range(n):
        for q in range(n):
            if t != q:
                d2[t, q], idx[t, q, 0], idx[t, q, 1], tie[t, q] = pair_record(vertices[t], vertices[q], bound2)
    return d2, idx, tie


def final_radius(parts, radius, restrict_by_radius):
    if radius is None:
        radius = np.inf
    if restrict_by_radius and parts:
        radius = max(2 * max(float(np.max(p.radii)) for p in parts), 0)
    return float(radius)


def plan(sizes, d2, idx, radii, radius, restrict_by_radius, used=None):
    """The merge plan: edges [(tree vertex, query vertex)] in the numbering of the concatenated parts.  sizes: vertices per part; radii:
    the parts' radii concatenated (f32).  used (a list): gets the (tree part, query part) of every record that decided a gap."""
    n = len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    radii = np.asarray(radii, dtype=np.float32)

    def gap(A, B):
        """cluster A as tree, B as query -> (np.float32 key, edge, deciding record)"""
        best = None
        for a, off_a in A:
            for b, off_b in B:
                if not np.isfinite(d2[a, b]):
                    continue
                kt, kq = int(idx[a, b, 0]), int(idx[a, b, 1])
                cand = (d2[a, b], kq + off_b, kt + off_a, int(first[a]) + kt, int(first[b]) + kq, (a, b))
                if best is None or cand[:3] < best[:3]:
                    best = cand
        if best is None:
            return np.float32(np.inf), None, None
        d = np.sqrt(np.float64(best[0]))
        if restrict_by_radius and d > (radii[best[3]] + radii[best[4]]):       # float32 sum against the float64 d
            d = np.inf
        return np.float32(d), (best[3], best[4]), best[5]

    clusters = [[(i, 0)] for i in range(n)]
    count = [int(s) for s in sizes]
    gaps = {(i, j): gap(clusters[i], clusters[j]) for i in range(n) for j in range(i + 1, n)}
    edges = []
    while len(clusters) > 1:
        m = len(clusters)
        key, i, j = min((gaps[(i, j)][0], i, j) for i in range(m) for j in range(i + 1, m))
        if not np.isfinite(key) or float(key) > radius:
            break
        edges.append(gaps[(i, j)][1])
        if used is not None:
            used.append(gaps[(i, j)][2])
        fused = clusters[i] + [(p, off + count[i]) for p, off in clusters[j]]
        rest = [k for k in range(m) if k not in (i, j)]
        renum = {old: new + 1 for new, old in enumerate(rest)}
        gaps = {(renum[p], renum[q]): v for (p, q), v in gaps.items() if p in renum and q in renum}
        count = [count[i] + count[j]] + [count[k] for k in rest]
        clusters = [fused] + [clusters[k] for k in rest]
        for k in range(1, len(clusters)):
            gaps[(0, k)] = gap(clusters[0], clusters[k])
    return np.asarray(edges, dtype=np.uint32).reshape(-1, 2)


def tables_of(parts, radius=np.inf, restrict_by_radius=False):
    """(sizes, d2, idx, tie, radii, final radius) of a group's parts"""
    r = final_radius(parts, radius, restrict_by_radius)
    d2, idx, tie = records([p.vertices for p in parts], (r + 0.000001) * (r + 0.000001))
    radii = np.concatenate([p.radii for p in parts]) if parts else np.zeros(0, np.float32)
    return [p.vertices.shape[0] for p in parts], d2, idx, tie, radii, r


def join(skeletons, radius=np.inf, restrict_by_radius=False):
    """-> (the Skeleton join_close_components_many returns for this group, whether a record that decided a merge carries a tree_tie,
    the number of records of the table that carry one)"""
    if radius is None:
        radius = np.inf
    if radius <= 0:
        raise ValueError("radius must be greater than zero: " + str(radius))
    parts = parts_of(skeletons)
    if not parts:
        return Skeleton(), False, 0
    if len(parts) == 1:
        return parts[0], False, 0
    sizes, d2, idx, tie, radii, r = tables_of(parts, radius, restrict_by_radius)
    used = []
    edges = plan(sizes, d2, idx, radii, r, restrict_by_radius, used)
    merged = Skeleton.simple_merge(parts)
    merged.edges = np.concatenate([merged.edges, edges])
    return merged.consolidate(remove_disconnected_vertices=True), any(tie[a, b] for a, b in used), int(tie.sum())


def fragments(seed, nfrag, nvert, extent, rmax, denom=1024, anisotropy=(1, 1, 1)):
    """nfrag random-walk paths of 2..nvert vertices as Skeletons: coordinates integer / denom * anisotropy as float32, steps in
    [-denom, denom] per axis from a start in [0, extent * denom); radii uniform in [0.5, rmax].  denom is a power of two, which keeps
    every float64 operation on the coordinates exact."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nfrag):
        k = int(rng.integers(2, nvert + 1))
        start = rng.integers(0, extent * denom, size=3)
        steps = rng.integers(-denom, denom + 1, size=(k - 1, 3))
        walk = np.concatenate([start[None], start[None] + np.cumsum(steps, axis=0)]).astype(np.float64)
        v = (walk / denom * np.asarray(anisotropy, dtype=np.float64)).astype(np.float32)
        e = np.stack([np.arange(k - 1), np.arange(1, k)], axis=1)
        out.append(Skeleton(v, e, rng.uniform(0.5, rmax, size=k).astype(np.float32), segid=1))
    return out


def same(a, b):
    """two Skeletons hold the same arrays"""
    return (a.vertices.shape == b.vertices.shape and np.array_equal(a.vertices, b.vertices) and np.array_equal(a.radii, b.radii)
            and a.edges.shape == b.edges.shape and np.array_equal(a.edges, b.edges))
